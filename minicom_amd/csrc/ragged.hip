// minicom_amd/csrc/ragged.hip -- reads of differing lengths (`minicom -p -V`).
//
// L is the modal sequence length of the file.  A record whose sequence is L bases long is EVEN and goes down the paths of the core
// untouched; every other record is ODD and its two lines go to side texts (odd.seq, odd.qual) back to back in input order; len.bin,
// one byte (length - 1) per record, says which is which.  Everything here works from the line index of mcom_decode_line_index, sixteen
// lanes per record as k_fastq_quality_rows does; untrusted text or members never take a kernel outside its buffers: flag and skip.
//
//   k_fastq_lengths      the record checks, len[first_record + r] = length - 1, and a 256-bin histogram of the lengths: bins of the
//                        workgroup in LDS, then one atomic add per bin that is not empty
//   k_ragged_marks       len -> (1 for an even record, the length for an odd one), two arrays for two exclusive scans
//   k_ragged_slots       the two scans -> slot[r]: rank among the even records, or offset into the odd text with bit 63 set
//   k_fastq_ragged_rows  line 4r + which of every record to its row (even) or to its place in the odd text (odd), re-checked
//   k_ragged_emit_sizes  bytes of every record of the output (0 and a flag for a record whose parts disagree), scanned into offsets
//   k_ragged_emit        the records back to back: four lines, or the read and a newline
#include "mcom_dev.hpp"

#define RG_THREADS 256
#define RG_G 16                                             // lanes per record
#define RG_NAME_MAX 255                                     // bytes behind the '@' or the '+' (name_model.hpp's NM_NAME_MAX)
#define RG_ODD ((uint64_t)1 << 63)

namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned blocks_for(uint64_t items) { return (unsigned)((items + RG_THREADS - 1) / RG_THREADS); }
}  // namespace

__device__ __forceinline__ bool rg_base_ok(uint8_t v) { return v == 'A' || v == 'C' || v == 'G' || v == 'T' || v == 'N'; }
__device__ __forceinline__ uint32_t rg_or16(uint32_t v)
{
#pragma unroll
	for (int o = RG_G / 2; o; o >>= 1) v |= __shfl_xor(v, o, RG_G);
	return v;
}

__global__ __launch_bounds__(RG_THREADS) void k_fastq_lengths(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ start, uint64_t first_record,
                                                              uint64_t n_records, uint8_t *__restrict__ len, unsigned long long *__restrict__ hist, uint32_t *__restrict__ flag)
{
	__shared__ uint32_t bins[256];
	bins[threadIdx.x] = 0;                                                     // (RG_THREADS == 256)
	__syncthreads();
	const uint64_t r = ((uint64_t)blockIdx.x * RG_THREADS + threadIdx.x) / RG_G;
	const uint32_t lane = threadIdx.x % RG_G;
	if (r < n_records) {                                                       // (all sixteen lanes of a record together)
		const uint64_t a = start[4 * r], b = start[4 * r + 1], c = start[4 * r + 2], d = start[4 * r + 3], e = start[4 * r + 4];
		uint32_t bad = 0;
		uint64_t sl = 0;
		if (!(a < b && b < c && c < d && d < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;     // (cannot be: the index is made of this text)
		else {
			if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
			if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
			sl = c - 1 - b;
			if (e - 1 - d != sl || sl < 1 || sl > 256) bad |= MCOM_FASTQ_F_LENGTH;
		}
		if (!(bad & MCOM_FASTQ_F_LENGTH))
			for (uint32_t j = lane; j < (uint32_t)sl; j += RG_G) {
				const uint8_t q = text[d + j];
				if (q < 33 || q > 126) bad |= MCOM_FASTQ_F_CHAR;
				if (!rg_base_ok(text[b + j])) bad |= MCOM_FASTQ_F_BASE;
			}
		bad = rg_or16(bad);
		if (lane == 0) {
			if (bad) { atomicOr(&flag[0], bad); atomicMin(&flag[1], (uint32_t)(first_record + r)); }
			else { len[first_record + r] = (uint8_t)(sl - 1); atomicAdd(&bins[sl - 1], 1u); }
		}
	}
	__syncthreads();
	const uint32_t mine = bins[threadIdx.x];
	if (mine) atomicAdd(&hist[threadIdx.x], (unsigned long long)mine);
}

extern "C" int mcom_fastq_lengths(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_line_start, uint64_t first_record, uint64_t n_records,
                                  uint8_t *d_len, uint64_t *d_hist, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || !d_hist || (n_records && (!d_text || !d_line_start || !d_len))) return mcom_fail(ctx, MCOM_E_ARG, "fastq_lengths: null pointer");
	if (first_record + n_records >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_lengths: %llu records from %llu", (unsigned long long)n_records, (unsigned long long)first_record);
	if (!n_records) return MCOM_OK;
	MCOM_LAUNCH(k_fastq_lengths, dim3(blocks_for(n_records * RG_G)), dim3(RG_THREADS), 0, ctx->stream, d_text, n_bytes, d_line_start, first_record, n_records, d_len,
	            (unsigned long long*)d_hist, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- the slots ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RG_THREADS) void k_ragged_marks(const uint8_t *__restrict__ len, uint64_t n, uint32_t L, uint64_t *__restrict__ even, uint64_t *__restrict__ odd)
{
	const uint64_t r = (uint64_t)blockIdx.x * RG_THREADS + threadIdx.x;
	if (r > n) return;
	const uint32_t l = r < n ? (uint32_t)len[r] + 1 : L;                       // entry n: the place of the two totals
	even[r] = r < n && l == L;
	odd[r] = l == L ? 0 : l;
}
__global__ __launch_bounds__(RG_THREADS) void k_ragged_slots(const uint8_t *__restrict__ len, uint64_t n, uint32_t L, const uint64_t *__restrict__ even, const uint64_t *__restrict__ odd,
                                                             uint64_t *__restrict__ slot)
{
	const uint64_t r = (uint64_t)blockIdx.x * RG_THREADS + threadIdx.x;
	if (r >= n) return;
	slot[r] = (uint32_t)len[r] + 1 == L ? even[r] : (odd[r] | RG_ODD);
}

extern "C" int mcom_ragged_index(mcom_ctx *ctx, const uint8_t *d_len, uint64_t n, uint32_t L, uint64_t *d_slot, uint64_t *n_even, uint64_t *n_odd, uint64_t *odd_bytes)
{
	if (!ctx) return MCOM_E_ARG;
	if (!n_even || !n_odd || !odd_bytes || (n && (!d_len || !d_slot))) return mcom_fail(ctx, MCOM_E_ARG, "ragged_index: null pointer");
	*n_even = *n_odd = *odd_bytes = 0;
	if (L < 1 || L > 256 || n >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "ragged_index: L %u, %llu records (L 1 .. 256, below 2^32 records)", L, (unsigned long long)n);
	if (!n) return MCOM_OK;
	Blocks B(ctx);
	uint64_t *d_even = nullptr, *d_odd = nullptr;
	MCOM_HIP(ctx, B.get(&d_even, (n + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_odd, (n + 1) * 8));
	MCOM_LAUNCH(k_ragged_marks, dim3(blocks_for(n + 1)), dim3(RG_THREADS), 0, ctx->stream, d_len, n, L, d_even, d_odd);
	MCOM_LAUNCH_CHECK(ctx);
	int rc;
	if ((rc = mcom_scan_u64(ctx, d_even, d_even, n + 1))) return rc;
	if ((rc = mcom_scan_u64(ctx, d_odd, d_odd, n + 1))) return rc;
	MCOM_LAUNCH(k_ragged_slots, dim3(blocks_for(n)), dim3(RG_THREADS), 0, ctx->stream, d_len, n, L, (const uint64_t*)d_even, (const uint64_t*)d_odd, d_slot);
	MCOM_LAUNCH_CHECK(ctx);
	uint64_t tot[2] = {0, 0};
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[0], d_even + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tot[1], d_odd + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*n_even = tot[0]; *n_odd = n - tot[0]; *odd_bytes = tot[1];
	return MCOM_OK;
}

// ---- text -> even rows and odd text -------------------------------------------------------------------------------------------------------
// A record's slot and length are read from tables that may come from a file (len.bin): the line's own length must agree with them, an
// even slot must lie below cap_rows, an odd one with its length inside odd_cap.  A flagged record is not copied.
__global__ __launch_bounds__(RG_THREADS) void k_fastq_ragged_rows(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ start, uint64_t first_record,
                                                                  uint64_t n_records, uint32_t which, uint32_t L, const uint8_t *__restrict__ len, const uint64_t *__restrict__ slot,
                                                                  uint8_t *__restrict__ rows, uint64_t pitch, uint64_t cap_rows, uint8_t *__restrict__ odd, uint64_t odd_cap,
                                                                  uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * RG_THREADS + threadIdx.x) / RG_G;
	const uint32_t lane = threadIdx.x % RG_G;
	if (r >= n_records) return;
	const uint64_t p = start[4 * r + which], q = start[4 * r + which + 1];
	uint32_t bad = 0, want = 0;
	uint8_t *dst = nullptr;
	if (!(p < q && q <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;                    // (cannot be: the index is made of this text)
	else {
		want = (uint32_t)len[first_record + r] + 1;
		const uint64_t s = slot[first_record + r], at = s & ~RG_ODD;
		const bool is_odd = (s & RG_ODD) != 0;
		if (q - 1 - p != want || is_odd == (want == L)) bad = MCOM_FASTQ_F_LENGTH;
		else if (!is_odd) { if (at >= cap_rows) bad = MCOM_FASTQ_F_LENGTH; else dst = rows + at * pitch; }
		else { if (at > odd_cap || want > odd_cap - at) bad = MCOM_FASTQ_F_LENGTH; else dst = odd + at; }
	}
	if (!bad)
		for (uint32_t j = lane; j < want; j += RG_G) {
			const uint8_t v = text[p + j];
			if (which == 1 ? !rg_base_ok(v) : (v < 33 || v > 126)) bad |= which == 1 ? MCOM_FASTQ_F_BASE : MCOM_FASTQ_F_CHAR; else dst[j] = v;
		}
	if (bad) { atomicOr(&flag[0], bad); atomicMin(&flag[1], (uint32_t)(first_record + r)); }
}

extern "C" int mcom_fastq_ragged_rows(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_line_start, uint64_t first_record, uint64_t n_records, int which,
                                      uint32_t L, const uint8_t *d_len, const uint64_t *d_slot, uint64_t n_total, uint8_t *d_rows, uint64_t pitch, uint64_t cap_rows, uint8_t *d_odd,
                                      uint64_t odd_cap, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || (n_records && (!d_text || !d_line_start || !d_len || !d_slot)) || (cap_rows && !d_rows) || (odd_cap && !d_odd)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_ragged_rows: null pointer");
	if ((which != 1 && which != 3) || L < 1 || L > 256 || pitch < L || n_total >= ((uint64_t)1 << 32) || first_record > n_total || n_records > n_total - first_record)
		return mcom_fail(ctx, MCOM_E_ARG, "fastq_ragged_rows: line %d, L %u, pitch %llu, %llu records from %llu of %llu", which, L, (unsigned long long)pitch, (unsigned long long)n_records,
		                 (unsigned long long)first_record, (unsigned long long)n_total);
	if (!n_records) return MCOM_OK;
	MCOM_LAUNCH(k_fastq_ragged_rows, dim3(blocks_for(n_records * RG_G)), dim3(RG_THREADS), 0, ctx->stream, d_text, n_bytes, d_line_start, first_record, n_records, (uint32_t)which, L,
	            d_len, d_slot, d_rows, pitch, cap_rows, d_odd, odd_cap, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// ---- even rows and odd texts -> records ---------------------------------------------------------------------------------------------------
// Where a record's read (and quality line) lies, checked against the tables' sizes: false when its parts disagree.
struct RgPlace { uint32_t l; bool is_odd; uint64_t at; };
__device__ __forceinline__ bool rg_place(const mcom_ragged_src &S, uint64_t i, RgPlace &P)
{
	P.l = (uint32_t)S.d_len[i] + 1;
	const uint64_t s = S.d_slot[i];
	P.is_odd = (s & RG_ODD) != 0; P.at = s & ~RG_ODD;
	if (P.is_odd == (P.l == S.L)) return false;
	return P.is_odd ? (P.at <= S.odd_bytes && P.l <= S.odd_bytes - P.at) : P.at < S.n_even;
}
// the record's piece of name text [at, end): two lines of at most 255 bytes, each with its newline
__device__ __forceinline__ bool rg_names_ok(const mcom_ragged_src &S, uint64_t i, uint64_t &at, uint64_t &end)
{
	at = S.d_rec_off[i]; end = S.d_rec_off[i + 1];
	return end >= at + 2 && end - at <= 2 * (uint64_t)RG_NAME_MAX + 2 && end <= S.names_bytes;
}
__device__ __forceinline__ uint32_t rg_digits(uint64_t v) { uint32_t nd = 1; for (; v >= 10; v /= 10) ++nd; return nd; }

__global__ __launch_bounds__(RG_THREADS) void k_ragged_emit_sizes(mcom_ragged_src S, uint64_t first, uint64_t count, uint64_t *__restrict__ size, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * RG_THREADS + threadIdx.x;
	if (r > count) return;
	uint64_t v = 0;
	if (r < count) {
		const uint64_t i = first + r;
		RgPlace P;
		uint64_t at = 0, end = 0;
		if (!rg_place(S, i, P) || (S.d_quals && S.d_names && !rg_names_ok(S, i, at, end))) atomicOr(flag, 1u);
		else if (!S.d_quals) v = (uint64_t)P.l + 1;
		else if (S.d_names) v = 2 * (uint64_t)P.l + 4 + (end - at);
		else v = 2 * (uint64_t)P.l + 6 + rg_digits(i + 1);
	}
	size[r] = v;
}

// the first newline of a record's piece of name text [at, end), found by the sixteen lanes of the record together (end when there is none)
__device__ __forceinline__ uint64_t rg_name_end(const uint8_t *names, uint64_t at, uint64_t end, uint32_t lane)
{
	uint32_t best = 0xFFFFFFFFu;
	for (uint64_t j = at + lane; j < end && best == 0xFFFFFFFFu; j += RG_G) if (names[j] == '\n') best = (uint32_t)(j - at);
#pragma unroll
	for (int o = RG_G / 2; o; o >>= 1) { const uint32_t other = __shfl_xor(best, o, RG_G); best = other < best ? other : best; }
	return best == 0xFFFFFFFFu ? end : at + best;
}

__global__ __launch_bounds__(RG_THREADS) void k_ragged_emit(mcom_ragged_src S, uint64_t first, uint64_t count, const uint64_t *__restrict__ off, uint8_t *__restrict__ out, uint64_t out_bytes,
                                                            uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * RG_THREADS + threadIdx.x) / RG_G;
	const uint32_t lane = threadIdx.x % RG_G;
	if (r >= count) return;
	// (all sixteen lanes of a record see the same tables and take the same way)
	const uint64_t i = first + r, o0 = off[r], o1 = off[r + 1];
	RgPlace P;
	if (!rg_place(S, i, P) || o1 < o0 || o1 > out_bytes) { if (lane == 0) atomicOr(flag, 1u); return; }
	const uint32_t l = P.l;
	const uint8_t *rd = P.is_odd ? S.d_odd_seq + P.at : S.d_reads + P.at * S.read_pitch;
	uint8_t *o = out + o0;
	if (!S.d_quals) {
		if (o1 - o0 != (uint64_t)l + 1) { if (lane == 0) atomicOr(flag, 1u); return; }
		for (uint32_t j = lane; j < l; j += RG_G) o[j] = rd[j];
		if (lane == 0) o[l] = '\n';
		return;
	}
	const uint8_t *ql = P.is_odd ? S.d_odd_qual + P.at : S.d_quals + P.at * S.qual_pitch;
	uint32_t nl, pl;                                                            // bytes behind the '@' and behind the '+'
	uint64_t at = 0, end = 0, mid = 0;
	if (S.d_names) {
		if (!rg_names_ok(S, i, at, end)) { if (lane == 0) atomicOr(flag, 1u); return; }
		mid = rg_name_end(S.d_names, at, end - 1, lane);                        // the name's newline; the text's is the piece's last byte
		if (mid >= end - 1 || S.d_names[end - 1] != '\n') { if (lane == 0) atomicOr(flag, 1u); return; }
		nl = (uint32_t)(mid - at); pl = (uint32_t)(end - 1 - at) - nl - 1;
	} else { nl = rg_digits(i + 1); pl = 0; }
	if (o1 - o0 != 2 * (uint64_t)l + 6 + nl + pl) { if (lane == 0) atomicOr(flag, 1u); return; }
	uint8_t *o_read = o + 1 + nl + 1, *o_plus = o_read + l + 1, *o_qual = o_plus + 1 + pl + 1;
	if (S.d_names) {
		for (uint32_t j = lane; j < nl; j += RG_G) o[1 + j] = S.d_names[at + j];
		for (uint32_t j = lane; j < pl; j += RG_G) o_plus[1 + j] = S.d_names[mid + 1 + j];
	} else if (lane == 0) {
		uint64_t v = i + 1;
		for (uint32_t k = nl; k > 0; --k) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
	}
	for (uint32_t j = lane; j < l; j += RG_G) { o_read[j] = rd[j]; o_qual[j] = ql[j]; }
	if (lane == 0) { o[0] = '@'; o[1 + nl] = '\n'; o_read[l] = '\n'; o_plus[0] = '+'; o_plus[1 + pl] = '\n'; o_qual[l] = '\n'; }
}

extern "C" int mcom_fastq_emit_ragged(mcom_ctx *ctx, const mcom_ragged_src *src, uint64_t first, uint64_t count, uint8_t *d_out, uint64_t cap, uint64_t *bytes)
{
	if (!ctx) return MCOM_E_ARG;
	if (!bytes || !src) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_ragged: null pointer");
	*bytes = 0;
	const mcom_ragged_src &S = *src;
	if (S.L < 1 || S.L > 256 || S.n >= ((uint64_t)1 << 32) || first > S.n || count > S.n - first || (S.n_even && S.read_pitch < S.L) || (S.d_quals && S.qual_pitch < S.L))
		return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_ragged: L %u, %llu records from %llu of %llu", S.L, (unsigned long long)count, (unsigned long long)first, (unsigned long long)S.n);
	if (!count) return MCOM_OK;
	if (!S.d_len || !S.d_slot || (S.n_even && !S.d_reads) || (S.odd_bytes && (!S.d_odd_seq || (S.d_quals && !S.d_odd_qual))) || (S.d_names && !S.d_rec_off))
		return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_ragged: null pointer");
	Blocks B(ctx);
	uint64_t *d_off = nullptr;
	uint32_t *d_flag = nullptr, flag = 0;
	MCOM_HIP(ctx, B.get(&d_off, (count + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_flag, 4));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	MCOM_LAUNCH(k_ragged_emit_sizes, dim3(blocks_for(count + 1)), dim3(RG_THREADS), 0, ctx->stream, S, first, count, d_off, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan_u64(ctx, d_off, d_off, count + 1);
	if (rc) return rc;
	uint64_t total = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&total, d_off + count, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_ragged: the lengths, the slots, the table sizes and the name offsets disagree");
	*bytes = total;
	if (!d_out) return MCOM_OK;
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "fastq_emit_ragged: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	MCOM_LAUNCH(k_ragged_emit, dim3(blocks_for(count * RG_G)), dim3(RG_THREADS), 0, ctx->stream, S, first, count, (const uint64_t*)d_off, d_out, total, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) { *bytes = 0; return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_ragged: the name text does not hold two lines per record"); }
	return MCOM_OK;
}
