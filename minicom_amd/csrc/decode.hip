// minicom_amd/csrc/decode.hip -- the stream files back into reads on the device: the inverse of streams.hip.
//
// The host decoder (host/mcom_decompress.cpp) walks three things in order: the contig headers of beg_pos.bin, the lines of the
// text streams, and the id / mate words of a member.  Here each of them is a prefix sum, after which a read is independent:
//   line index    '\n' counted per 4 KiB tile, scanned, the start of line m scattered                     (k_dc_count_nl, k_dc_scatter_nl)
//   member table  member -> contig by bisection of the contigs' first members, begin position = difference of two entries of one
//                 scan of the 16-bit deltas, contig length = last position + L, scanned to the contig's base offset in ref.bin
//                                                                                                        (k_dc_member_delta, k_dc_member_pos)
//   destinations  -p: list ids = inclusive scan of the deltas; member ids = difference of two entries of a scan of ids.bin, from the
//                 first member of the same begin position; paired end: the file bits scanned              (k_dc_member_ids, k_dc_pe_dest)
//   line check    every line parsed once by one lane with the host decoder's rules, before anything is decoded   (k_dc_check_lines)
//   decode        sixteen lanes per read: the reference window (or a constant base) into an LDS row, the literals of the line patched
//                 in, the row stored -- reverse-complemented when the direction bit is set -- as aligned 16-byte pieces (k_dc_reads)
//   window        a range of rows alone: the placement check over all reads, a compacted list of the reads whose destination lies in
//                 the window, the decode over that list                                        (k_dc_check_dest, k_dc_select, k_dc_reads_sel)
// The only serial part is the chain of contig headers ("header c + 1 sits 4 + 2 num bytes behind header c"): mcom_decode_walk_headers
// follows it on the host, four bytes read per contig.
//
// The archive is untrusted: whatever becomes an index is compared with the size of what it indexes; a violation raises a bit of the
// caller's flag word (atomicOr) and the access is skipped.
#include "mcom_dev.hpp"
#include <cstring>

#define DC_THREADS 256
#define DC_TILE 4096            // bytes of text per workgroup: 16 per lane
#define DC_G 16                 // lanes per read in k_dc_reads
#define DC_RPB (DC_THREADS / DC_G)
#define DC_PITCH 272            // bytes of an LDS row: 256 bases + slack, a multiple of 16

// ---- line index -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t dc_nl_mask(const uint8_t *__restrict__ text, uint64_t n, uint64_t at, bool aligned)
{
	uint32_t m = 0;
	if (at >= n) return 0;
	if (aligned && at + 16 <= n) {
		const uint4 q = *(const uint4*)(text + at);
		const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
		for (int u = 0; u < 4; ++u)
#pragma unroll
			for (int b = 0; b < 4; ++b) if (((w[u] >> (8 * b)) & 0xFFu) == (uint32_t)'\n') m |= 1u << (4 * u + b);
	} else {
		for (int j = 0; j < 16 && at + j < n; ++j) if (text[at + j] == (uint8_t)'\n') m |= 1u << j;
	}
	return m;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_count_nl(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ cnt)
{
	__shared__ uint32_t ws[DC_THREADS / 64];
	const bool aligned = (((uintptr_t)text) & 15) == 0;
	const uint64_t at = (uint64_t)blockIdx.x * DC_TILE + (uint64_t)threadIdx.x * 16;
	uint32_t c = __popc(dc_nl_mask(text, n, at, aligned));
#pragma unroll
	for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
	if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) { uint32_t t = 0; for (int q = 0; q < DC_THREADS / 64; ++q) t += ws[q]; cnt[blockIdx.x] = t; }
}

// line_start[m] = byte behind the m-th '\n' (line_start[0] = 0): line m is [line_start[m], line_start[m + 1] - 1)
__global__ __launch_bounds__(DC_THREADS) void k_dc_scatter_nl(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ base,
                                                              uint64_t *__restrict__ line_start, uint64_t n_lines, uint32_t *__restrict__ flag)
{
	__shared__ uint32_t ws[DC_THREADS / 64];
	const bool aligned = (((uintptr_t)text) & 15) == 0;
	const uint64_t at = (uint64_t)blockIdx.x * DC_TILE + (uint64_t)threadIdx.x * 16;
	uint32_t m = dc_nl_mask(text, n, at, aligned);
	const uint32_t c = __popc(m);
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	uint32_t inc = c;
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) { const uint32_t t = __shfl_up(inc, s, 64); if (lane >= s) inc += t; }
	if (lane == 63) ws[wv] = inc;
	__syncthreads();
	uint32_t add = 0;
	for (int q = 0; q < wv; ++q) add += ws[q];
	uint64_t k = base[blockIdx.x] + add + inc - c;
	if (blockIdx.x == 0 && threadIdx.x == 0) line_start[0] = 0;
	while (m) {
		const int j = __ffs(m) - 1; m &= m - 1;
		++k;
		if (k <= n_lines) line_start[k] = at + j + 1; else atomicOr(flag, MCOM_DECODE_F_BOUNDS);
	}
}

// ---- member table -----------------------------------------------------------------------------------------------------------
// contig of member q: the last c with moff[c] <= q (empty contigs share their successor's first member and are stepped over)
__device__ __forceinline__ uint64_t dc_contig_of(const uint64_t *__restrict__ moff, uint64_t n_contigs, uint64_t q)
{
	uint64_t lo = 0, hi = n_contigs;                                       // answer in [lo, hi)
	while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (moff[mid] <= q) lo = mid; else hi = mid; }
	return lo;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_member_delta(const uint8_t *__restrict__ bpos, uint64_t bpos_bytes, const uint64_t *__restrict__ moff,
                                                                uint64_t n_contigs, uint64_t n_members, uint32_t *__restrict__ cid, uint64_t *__restrict__ dl,
                                                                uint32_t *__restrict__ flag)
{
	const uint64_t q = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (q >= n_members) return;
	const uint64_t c = dc_contig_of(moff, n_contigs, q);
	const uint64_t o = 4 * (c + 1) + 2 * q;                                // the header of contig c sits at 4 c + 2 moff[c]
	uint64_t d = 0;
	if (moff[c] > q || moff[c + 1] <= q || o + 2 > bpos_bytes) atomicOr(flag, MCOM_DECODE_F_BOUNDS);
	else d = (uint64_t)bpos[o] | ((uint64_t)bpos[o + 1] << 8);
	cid[q] = (uint32_t)c;
	dl[q] = d;
}

// e = exclusive scan of the deltas over all members (n_members + 1 entries): the begin position of q is e[q + 1] - e[first of its contig]
__global__ __launch_bounds__(DC_THREADS) void k_dc_member_pos(const uint64_t *__restrict__ e, const uint64_t *__restrict__ moff, const uint32_t *__restrict__ cid,
                                                              uint64_t n_members, int L, uint32_t *__restrict__ pos, uint64_t *__restrict__ clen,
                                                              uint32_t *__restrict__ flag)
{
	const uint64_t q = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (q >= n_members) return;
	const uint64_t c = cid[q];
	uint64_t first = moff[c]; if (first > q) first = q;                    // (flagged by k_dc_member_delta)
	uint64_t p = e[q + 1] - e[first];
	if (p + (uint64_t)L > 0x7FFFFFFFull) { atomicOr(flag, MCOM_DECODE_F_BOUNDS); p = 0; }
	pos[q] = (uint32_t)p;
	if (q + 1 == moff[c + 1]) clen[c] = p + (uint64_t)L;                   // positions do not decrease: the last member ends the contig
}

// ---- destinations -----------------------------------------------------------------------------------------------------------
// out[i] = in[i]; pad: out has n + 1 entries, the last one zero (an exclusive scan then leaves the total there)
__global__ __launch_bounds__(DC_THREADS) void k_dc_widen_u32(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out, int pad)
{
	const uint64_t i = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (i < n) out[i] = in[i]; else if (i == n && pad) out[i] = 0;
}
__global__ __launch_bounds__(DC_THREADS) void k_dc_add_u32(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (i < n) out[i] += in[i];
}

// ids.bin: a member carries its id when it is the first of its contig or begins at a new position, else the difference to the
// member before it: id = sum of the words from the first member of the same begin position on (mod 2^32).  e = exclusive scan.
__global__ __launch_bounds__(DC_THREADS) void k_dc_member_ids(const uint64_t *__restrict__ e, const uint64_t *__restrict__ moff, const uint32_t *__restrict__ cid,
                                                              const uint32_t *__restrict__ pos, uint64_t n_members, uint64_t *__restrict__ dest)
{
	const uint64_t q = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (q >= n_members) return;
	uint64_t lo = moff[cid[q]]; if (lo > q) lo = q;
	const uint32_t p = pos[q];
	uint64_t hi = q;                                                       // first h in [lo, q] with pos[h] == p (positions do not decrease)
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (pos[mid] < p) lo = mid + 1; else hi = mid; }
	dest[q] = (e[q + 1] - e[lo]) & 0xFFFFFFFFull;
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_bits_u64(const uint8_t *__restrict__ bits, uint64_t bytes, uint64_t bit0, uint64_t n, uint64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (i > n) return;
	const uint64_t b = bit0 + i;
	out[i] = (i < n && (b >> 3) < bytes) ? (uint64_t)((bits[b >> 3] >> (b & 7)) & 1u) : 0ull;
}
// ones = exclusive scan of the file bits.  A read of the first file goes to the next row of output 1, a read of the second file to
// the row its peids word names of output 2 (rows half .. 2 half - 1 of the table).
__global__ __launch_bounds__(DC_THREADS) void k_dc_pe_dest(const uint64_t *__restrict__ ones, uint64_t n, const uint32_t *__restrict__ peids, uint64_t n_peids,
                                                           uint64_t zero_base, uint64_t half, uint64_t *__restrict__ dest, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (r >= n) return;
	const uint64_t ob = ones[r];
	uint64_t d = ~0ull;
	if (ones[r + 1] != ob) {
		if (ob >= n_peids) atomicOr(flag, MCOM_DECODE_F_BOUNDS);
		else { const uint64_t v = peids[ob]; if (v >= half) atomicOr(flag, MCOM_DECODE_F_DEST); else d = half + v; }
	} else {
		const uint64_t row = zero_base + r - ob;
		if (row >= half) atomicOr(flag, MCOM_DECODE_F_DEST); else d = row;
	}
	dest[r] = d;
}

// ---- lines ------------------------------------------------------------------------------------------------------------------
// decode_line's acceptance (host/mcom_decompress.cpp): letters are literal bases, a decimal number a run taken from the reference,
// never more than L bases; anything else refuses the archive.  verbatim: the line is the read, exactly L bytes.
__global__ __launch_bounds__(DC_THREADS) void k_dc_check_lines(const uint8_t *__restrict__ text, uint64_t text_bytes, const uint64_t *__restrict__ line_start,
                                                               uint64_t n, int L, int verbatim, uint32_t *__restrict__ flag)
{
	const uint64_t m = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (m >= n) return;
	const uint64_t s = line_start[m], e1 = line_start[m + 1];
	if (e1 <= s || e1 > text_bytes) { atomicOr(flag, MCOM_DECODE_F_BOUNDS); return; }
	const uint64_t e = e1 - 1;
	if (verbatim) { if (e - s != (uint64_t)L) atomicOr(flag, MCOM_DECODE_F_LINE); return; }
	long at = 0, eq = 0;
	bool ok = true;
	for (uint64_t i = s; i < e && ok; ++i) {
		const uint8_t ch = text[i];
		if (ch >= 'A' && ch <= 'Z') { if (at + eq + 1 > (long)L) ok = false; at += eq + 1; eq = 0; }
		else if (ch >= '0' && ch <= '9') { eq = eq * 10 + (ch - '0'); if (eq > (long)L) ok = false; }
		else ok = false;
	}
	if (!ok) atomicOr(flag, MCOM_DECODE_F_LINE);
}

// ---- decode -----------------------------------------------------------------------------------------------------------------
struct DcReads {
	const uint8_t *text; uint64_t text_bytes; const uint64_t *line_start; int verbatim;       // text == nullptr: no line, the reference as it is
	const uint8_t *ref; uint64_t ref_bytes; int ref_const;                                     // ref == nullptr: L times ref_const
	const uint32_t *cid; const uint32_t *pos; const uint64_t *coff; uint64_t n_contigs;       // cid == nullptr: read m is bases [m L, m L + L)
	const uint8_t *dir; uint64_t dir_bytes;                                                    // dir == nullptr: never reversed
	const uint64_t *dest; uint64_t dest0;                                                      // dest == nullptr: row dest0 + m
	uint64_t n; int L;
	uint8_t *out; uint64_t n_rows; uint32_t *seen; uint32_t *flag;
};

__device__ __forceinline__ uint8_t dc_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N'; }

// Steps 1 to 3 of a read's decode, the body k_dc_reads and k_dc_agree share: the reference window into the LDS row, the literals of the
// line laid over it, the destination row into s_dest[g] (~0: none).  Every thread of the workgroup calls it (two barriers).  WIN (the
// agreement mask): only a contig member has a window, whose places must also lie inside the coverage array
// (cov_bases); `win` says per column "still the window byte" -- a literal clears it unless it equals the window byte -- and every other
// read gets a row of N that agrees with nothing; no duplicate check (the rows' decoder has made it).
template <bool WIN>
__device__ __forceinline__ void dc_row_steps(const DcReads &a, uint64_t m, bool live, int g, int lane, uint8_t *row, uint8_t *win, uint64_t cov_bases, uint64_t *s_dest,
                                             bool &have, uint64_t &off)
{
	const int L = a.L;
	have = false; off = 0;
	// 1. the reference window
	if (live) {
		if (a.ref && (!WIN || a.cid)) {
			have = true;
			if (a.cid) { const uint64_t c = a.cid[m]; if (c < a.n_contigs) off = a.coff[c] + a.pos[m]; else have = false; }
			else off = m * (uint64_t)L;
			if (have && (off + (uint64_t)L > 4 * a.ref_bytes || (WIN && off + (uint64_t)L > cov_bases))) have = false;
			if (!have && lane == 0) atomicOr(a.flag, MCOM_DECODE_F_BOUNDS);
		}
		if (have) {
			for (int p = lane * 4; p < L; p += DC_G * 4) {
				const uint64_t b = off + p, by = b >> 2; const int sh = 2 * (int)(b & 3);
				uint32_t v = by < a.ref_bytes ? a.ref[by] : 0u;
				if (sh && by + 1 < a.ref_bytes) v |= (uint32_t)a.ref[by + 1] << 8;
				v >>= sh;
				uint32_t w = 0;
#pragma unroll
				for (int j = 0; j < 4; ++j) w |= (uint32_t)(uint8_t)"ACGT"[(v >> (2 * j)) & 3u] << (8 * j);
				*(uint32_t*)(row + p) = w;
				if (WIN) *(uint32_t*)(win + p) = 0x01010101u;
			}
		} else {
			const uint32_t ch = WIN ? (uint32_t)'N' : a.ref ? (uint32_t)'A' : (uint32_t)(uint8_t)a.ref_const;
			for (int p = lane * 4; p < L; p += DC_G * 4) { *(uint32_t*)(row + p) = ch * 0x01010101u; if (WIN) *(uint32_t*)(win + p) = 0u; }
		}
	}
	__syncthreads();
	// 2. the line: its literals over the window (one lane: a line is a few bytes), or the line itself
	if (live && a.text && (!WIN || (have && !a.verbatim))) {
		const uint64_t s = a.line_start[m], e1 = a.line_start[m + 1];
		if (e1 <= s || e1 > a.text_bytes) { if (lane == 0) atomicOr(a.flag, MCOM_DECODE_F_BOUNDS); }
		else if (a.verbatim) {
			if (e1 - 1 - s != (uint64_t)L) { if (lane == 0) atomicOr(a.flag, MCOM_DECODE_F_LINE); }
			else for (int p = lane; p < L; p += DC_G) row[p] = a.text[s + p];
		} else if (lane == 0) {
			long at = 0, eq = 0;
			bool ok = true;
			for (uint64_t i = s; i + 1 < e1 && ok; ++i) {
				const uint8_t ch = a.text[i];
				if (ch >= 'A' && ch <= 'Z') { if (at + eq + 1 > (long)L) ok = false; else { at += eq; eq = 0; if (WIN && row[at] != ch) win[at] = 0; row[at++] = ch; } }
				else if (ch >= '0' && ch <= '9') { eq = eq * 10 + (ch - '0'); if (eq > (long)L) ok = false; }
				else ok = false;
			}
			if (!ok) atomicOr(a.flag, MCOM_DECODE_F_LINE);
		}
	}
	// 3. where it goes
	if (live && lane == 0) {
		uint64_t d = a.dest ? a.dest[m] : a.dest0 + m;
		if (d >= a.n_rows) { atomicOr(a.flag, MCOM_DECODE_F_DEST); d = ~0ull; }
		else if (!WIN && a.seen) {
			const uint32_t bit = 1u << (d & 31);
			if (atomicOr(a.seen + (d >> 5), bit) & bit) { atomicOr(a.flag, MCOM_DECODE_F_DUP); d = ~0ull; }
		}
		s_dest[g] = d;
	}
	__syncthreads();
}

// Steps 1 to 4 of read m, for the sixteen lanes of group g: the body of k_dc_reads and of k_dc_reads_sel.  The row is stored at row
// (destination - row0) of a.out; a destination below row0 is skipped (k_dc_reads: row0 = 0).  Every thread of the workgroup calls it.
__device__ __forceinline__ void dc_read_body(const DcReads &a, uint64_t m, bool live, uint64_t row0, int g, int lane, uint8_t *row, uint64_t *s_dest)
{
	const int L = a.L;
	bool have; uint64_t off;
	dc_row_steps<false>(a, m, live, g, lane, row, nullptr, 0, s_dest, have, off);
	if (!live) return;
	uint64_t d = s_dest[g];
	if (d == ~0ull || d < row0) return;
	d -= row0;
	bool rev = false;
	if (a.dir && (m >> 3) < a.dir_bytes) rev = (a.dir[m >> 3] >> (m & 7)) & 1u;
	// 4. the row, L characters and the newline, as the aligned 16-byte pieces of the output it covers
	uint8_t *dst = a.out + d * (uint64_t)(L + 1);
	const int lead = (int)(((uintptr_t)dst) & 15);
	const int n_pieces = (lead + L + 1 + 15) >> 4;
	auto chr = [&](int i) -> uint8_t { return i == L ? (uint8_t)'\n' : rev ? dc_comp(row[L - 1 - i]) : row[i]; };
	for (int k = lane; k < n_pieces; k += DC_G) {
		const int s = k * 16 - lead;
		if (s >= 0 && s + 16 <= L + 1) {
			uint32_t w[4];
#pragma unroll
			for (int u = 0; u < 4; ++u) {
				uint32_t x = 0;
#pragma unroll
				for (int j = 0; j < 4; ++j) x |= (uint32_t)chr(s + 4 * u + j) << (8 * j);
				w[u] = x;
			}
			*(uint4*)(dst + s) = make_uint4(w[0], w[1], w[2], w[3]);
		} else {
			for (int j = 0; j < 16; ++j) { const int i = s + j; if (i >= 0 && i <= L) dst[i] = chr(i); }
		}
	}
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_reads(const DcReads a)
{
	__shared__ __align__(16) uint8_t s_row[DC_RPB][DC_PITCH];
	__shared__ uint64_t s_dest[DC_RPB];
	const int g = threadIdx.x / DC_G, lane = threadIdx.x % DC_G;
	const uint64_t m = (uint64_t)blockIdx.x * DC_RPB + g;
	dc_read_body(a, m, m < a.n, 0, g, lane, s_row[g], s_dest);
}

// ---- a window of rows ---------------------------------------------------------------------------------
//   placement  the check of step 3 on its own, over ALL reads of a source: one thread per read                      (k_dc_check_dest)
//   selection  one thread per read: is its destination inside [win_first, win_first + win_count)?  The reads that are get a place in
//              a compacted list, one atomic per wave from a ballot; the order of the list does not matter            (k_dc_select)
//   decode     the body of k_dc_reads over the list: group k takes read sel[k], its row is destination - win_first.  The grid covers
//              min(n, win_count) groups -- a row of the window is named by at most one read of an archive that has passed the
//              placement check -- and a group beyond the list's length, which the kernel reads from the device, exits (k_dc_reads_sel)
__global__ __launch_bounds__(DC_THREADS) void k_dc_check_dest(const uint64_t *__restrict__ dest, uint64_t dest0, uint64_t n, uint64_t n_rows,
                                                              uint32_t *__restrict__ seen, uint32_t *__restrict__ flag)
{
	const uint64_t m = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (m >= n) return;
	const uint64_t d = dest ? dest[m] : dest0 + m;
	if (d >= n_rows) { atomicOr(flag, MCOM_DECODE_F_DEST); return; }
	const uint32_t bit = 1u << (d & 31);
	if (atomicOr(seen + (d >> 5), bit) & bit) atomicOr(flag, MCOM_DECODE_F_DUP);
}

// sel: room for `cap` read indices; *count: cleared by the caller.  More reads inside the window than `cap` (a row named twice: cap is
// at least the window's rows, or all reads) raise F_DUP and get no place.
__global__ __launch_bounds__(DC_THREADS) void k_dc_select(const uint64_t *__restrict__ dest, uint64_t dest0, uint64_t n, uint64_t win_first, uint64_t win_count,
                                                          uint64_t *__restrict__ sel, uint64_t cap, unsigned long long *__restrict__ count, uint32_t *__restrict__ flag)
{
	const uint64_t m = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	const int lane = threadIdx.x & 63;
	bool in = false;
	if (m < n) { const uint64_t d = dest ? dest[m] : dest0 + m; in = d >= win_first && d - win_first < win_count; }
	const unsigned long long mask = __ballot(in);
	if (!mask) return;
	const int leader = __ffsll(mask) - 1;
	unsigned long long base = 0;
	if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
	base = __shfl(base, leader, 64);
	if (!in) return;
	const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1));
	if (at < cap) sel[at] = m; else atomicOr(flag, MCOM_DECODE_F_DUP);
}

// a.n_rows = win_first + win_count and a.seen = nullptr: step 3 flags a destination behind the window, and the list holds none
__global__ __launch_bounds__(DC_THREADS) void k_dc_reads_sel(const DcReads a, const uint64_t *__restrict__ sel, const unsigned long long *__restrict__ count, uint64_t cap,
                                                             uint64_t win_first)
{
	__shared__ __align__(16) uint8_t s_row[DC_RPB][DC_PITCH];
	__shared__ uint64_t s_dest[DC_RPB];
	const int g = threadIdx.x / DC_G, lane = threadIdx.x % DC_G;
	const uint64_t k = (uint64_t)blockIdx.x * DC_RPB + g;
	uint64_t n_sel = *count; if (n_sel > cap) n_sel = cap;
	bool live = k < n_sel;
	const uint64_t m = live ? sel[k] : 0;
	if (m >= a.n) live = false;                                            // (cannot be: the list is k_dc_select's)
	dc_read_body(a, m, live, win_first, g, lane, s_row[g], s_dest);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------
static inline unsigned dc_blocks(uint64_t n) { return (unsigned)((n + DC_THREADS - 1) / DC_THREADS); }
#define DC_MAX_ITEMS (1ull << 38)     // items per call: keeps every grid below 2^31 workgroups

extern "C" int mcom_decode_walk_headers(const uint8_t *h_bpos, uint64_t bytes, uint64_t *h_moff, uint64_t cap_contigs, uint64_t *n_contigs, uint64_t *n_members)
{
	if ((!h_bpos && bytes) || !n_contigs || !n_members) return MCOM_E_ARG;
	uint64_t pp = 0, nc = 0, nm = 0;
	while (pp + 4 <= bytes) {
		uint32_t num; memcpy(&num, h_bpos + pp, 4);
		if (2 * (uint64_t)num > bytes - pp - 4) return MCOM_E_ARG;         // the contig's deltas leave the file
		if (h_moff) { if (nc >= cap_contigs) return MCOM_E_OVERFLOW; h_moff[nc] = nm; }
		pp += 4 + 2 * (uint64_t)num; nm += num; ++nc;
	}
	if (h_moff) h_moff[nc] = nm;
	*n_contigs = nc; *n_members = nm;
	return MCOM_OK;
}

extern "C" int mcom_decode_line_index(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint64_t *d_line_start, uint64_t cap_lines,
                                      uint64_t *h_n_lines, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!h_n_lines || (n_bytes && !d_text) || (d_line_start && !d_flag)) return mcom_fail(ctx, MCOM_E_ARG, "decode_line_index: null pointer");
	if (n_bytes >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "decode_line_index: %llu bytes", (unsigned long long)n_bytes);
	*h_n_lines = 0;
	if (n_bytes == 0) { if (d_line_start) MCOM_HIP(ctx, hipMemsetAsync(d_line_start, 0, 8, ctx->stream)); return MCOM_OK; }
	const uint64_t tiles = (n_bytes + DC_TILE - 1) / DC_TILE;
	uint64_t *cnt = nullptr;
	MCOM_HIP(ctx, mcom_dmalloc(&cnt, (tiles + 1) * 8));
	mcom_dfree_later(ctx, cnt);
	MCOM_HIP(ctx, hipMemsetAsync(cnt + tiles, 0, 8, ctx->stream));
	MCOM_LAUNCH(k_dc_count_nl, dim3((unsigned)tiles), dim3(DC_THREADS), 0, ctx->stream, d_text, n_bytes, cnt);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan64(ctx, cnt, cnt, tiles + 1, nullptr);
	if (rc) return rc;
	uint64_t total = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&total, cnt + tiles, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipStreamSynchronize(ctx->stream));
	*h_n_lines = total;
	if (!d_line_start) { MCOM_HIP(ctx, mcom_stream_sync(ctx)); return MCOM_OK; }
	if (total > cap_lines) return mcom_fail(ctx, MCOM_E_OVERFLOW, "decode_line_index: %llu lines, room for %llu", (unsigned long long)total, (unsigned long long)cap_lines);
	MCOM_LAUNCH(k_dc_scatter_nl, dim3((unsigned)tiles), dim3(DC_THREADS), 0, ctx->stream, d_text, n_bytes, (const uint64_t*)cnt, d_line_start, total, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_decode_member_table(mcom_ctx *ctx, const uint8_t *d_bpos, uint64_t bpos_bytes, const uint64_t *d_moff, uint64_t n_contigs, uint64_t n_members,
                                        int L, uint32_t *d_cid, uint32_t *d_pos, uint64_t *d_coff, uint64_t *h_ref_bases, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!h_ref_bases || !d_coff || !d_flag || L < 1 || L > 256) return mcom_fail(ctx, MCOM_E_ARG, "decode_member_table: bad argument");
	if (n_members && (!d_bpos || !d_moff || !d_cid || !d_pos || n_contigs == 0)) return mcom_fail(ctx, MCOM_E_ARG, "decode_member_table: null pointer");
	if (n_members >= DC_MAX_ITEMS || n_contigs >= (1ull << 32)) return mcom_fail(ctx, MCOM_E_ARG, "decode_member_table: too many members or contigs");
	*h_ref_bases = 0;
	MCOM_HIP(ctx, hipMemsetAsync(d_coff, 0, (n_contigs + 1) * 8, ctx->stream));
	if (n_members) {
		uint64_t *e = nullptr;
		MCOM_HIP(ctx, mcom_dmalloc(&e, (n_members + 1) * 8));
		mcom_dfree_later(ctx, e);
		MCOM_HIP(ctx, hipMemsetAsync(e + n_members, 0, 8, ctx->stream));
		MCOM_LAUNCH(k_dc_member_delta, dim3(dc_blocks(n_members)), dim3(DC_THREADS), 0, ctx->stream, d_bpos, bpos_bytes, d_moff, n_contigs, n_members, d_cid, e, d_flag);
		MCOM_LAUNCH_CHECK(ctx);
		int rc = mcom_scan64(ctx, e, e, n_members + 1, nullptr);
		if (rc) return rc;
		MCOM_LAUNCH(k_dc_member_pos, dim3(dc_blocks(n_members)), dim3(DC_THREADS), 0, ctx->stream, (const uint64_t*)e, d_moff, (const uint32_t*)d_cid, n_members, L, d_pos, d_coff, d_flag);
		MCOM_LAUNCH_CHECK(ctx);
		rc = mcom_scan64(ctx, d_coff, d_coff, n_contigs + 1, nullptr);
		if (rc) return rc;
		MCOM_HIP(ctx, hipMemcpyAsync(h_ref_bases, d_coff + n_contigs, 8, hipMemcpyDeviceToHost, ctx->stream));
	}
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_decode_list_ids(mcom_ctx *ctx, const uint32_t *d_delta, uint64_t n, uint64_t *d_dest)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0) return MCOM_OK;
	if (!d_delta || !d_dest || n >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "decode_list_ids: bad argument");
	MCOM_LAUNCH(k_dc_widen_u32, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, d_delta, n, d_dest, 0);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan64(ctx, d_dest, d_dest, n, nullptr);
	if (rc) return rc;
	MCOM_LAUNCH(k_dc_add_u32, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, d_delta, n, d_dest);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

extern "C" int mcom_decode_member_ids(mcom_ctx *ctx, const uint32_t *d_ids, uint64_t n_members, const uint64_t *d_moff, const uint32_t *d_cid, const uint32_t *d_pos,
                                      uint64_t *d_dest)
{
	if (!ctx) return MCOM_E_ARG;
	if (n_members == 0) return MCOM_OK;
	if (!d_ids || !d_moff || !d_cid || !d_pos || !d_dest || n_members >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "decode_member_ids: bad argument");
	uint64_t *e = nullptr;
	MCOM_HIP(ctx, mcom_dmalloc(&e, (n_members + 1) * 8));
	mcom_dfree_later(ctx, e);
	MCOM_LAUNCH(k_dc_widen_u32, dim3(dc_blocks(n_members + 1)), dim3(DC_THREADS), 0, ctx->stream, d_ids, n_members, e, 1);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan64(ctx, e, e, n_members + 1, nullptr);
	if (rc) return rc;
	MCOM_LAUNCH(k_dc_member_ids, dim3(dc_blocks(n_members)), dim3(DC_THREADS), 0, ctx->stream, (const uint64_t*)e, d_moff, d_cid, d_pos, n_members, d_dest);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

extern "C" int mcom_decode_pe_dest(mcom_ctx *ctx, const uint8_t *d_fbits, uint64_t fb_bytes, uint64_t bit0, uint64_t n, const uint32_t *d_peids, uint64_t n_peids,
                                   uint64_t zero_base, uint64_t half, uint64_t *d_dest, uint64_t *h_ones, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!h_ones || !d_flag) return mcom_fail(ctx, MCOM_E_ARG, "decode_pe_dest: null pointer");
	*h_ones = 0;
	if (n == 0) return MCOM_OK;
	if (!d_dest || (fb_bytes && !d_fbits) || (n_peids && !d_peids) || n >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "decode_pe_dest: bad argument");
	uint64_t *e = nullptr;
	MCOM_HIP(ctx, mcom_dmalloc(&e, (n + 1) * 8));
	mcom_dfree_later(ctx, e);
	MCOM_LAUNCH(k_dc_bits_u64, dim3(dc_blocks(n + 1)), dim3(DC_THREADS), 0, ctx->stream, d_fbits, fb_bytes, bit0, n, e);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan64(ctx, e, e, n + 1, nullptr);
	if (rc) return rc;
	MCOM_LAUNCH(k_dc_pe_dest, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, (const uint64_t*)e, n, d_peids, n_peids, zero_base, half, d_dest, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(h_ones, e + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_decode_check_lines(mcom_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_line_start, uint64_t n, int L, int verbatim,
                                       uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0) return MCOM_OK;
	if (!d_text || !d_line_start || !d_flag || L < 1 || L > 256 || n >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "decode_check_lines: bad argument");
	MCOM_LAUNCH(k_dc_check_lines, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, d_text, text_bytes, d_line_start, n, L, verbatim, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

static void dc_fill(DcReads &a, const mcom_decode_src *src, uint64_t n, int L, const uint64_t *d_dest, uint64_t dest0, uint8_t *d_out, uint64_t n_rows, uint32_t *d_seen, uint32_t *d_flag)
{
	a.text = src->d_text; a.text_bytes = src->text_bytes; a.line_start = src->d_line_start; a.verbatim = src->verbatim;
	a.ref = src->d_ref; a.ref_bytes = src->ref_bytes; a.ref_const = src->ref_const;
	a.cid = src->d_cid; a.pos = src->d_pos; a.coff = src->d_coff; a.n_contigs = src->n_contigs;
	a.dir = src->d_dir; a.dir_bytes = src->dir_bytes;
	a.dest = d_dest; a.dest0 = dest0; a.n = n; a.L = L; a.out = d_out; a.n_rows = n_rows; a.seen = d_seen; a.flag = d_flag;
}

extern "C" int mcom_decode_reads(mcom_ctx *ctx, const mcom_decode_src *src, uint64_t n, int L, const uint64_t *d_dest, uint64_t dest0,
                                 uint8_t *d_out, uint64_t n_rows, uint32_t *d_seen, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0) return MCOM_OK;
	if (!src || !d_out || !d_flag || L < 1 || L > 256 || n >= (1ull << 34)) return mcom_fail(ctx, MCOM_E_ARG, "decode_reads: bad argument");
	if (src->d_text && !src->d_line_start) return mcom_fail(ctx, MCOM_E_ARG, "decode_reads: a text without its line index");
	if (src->d_cid && (!src->d_ref || !src->d_pos || !src->d_coff)) return mcom_fail(ctx, MCOM_E_ARG, "decode_reads: a member table without its reference");
	DcReads a;
	dc_fill(a, src, n, L, d_dest, dest0, d_out, n_rows, d_seen, d_flag);
	MCOM_LAUNCH(k_dc_reads, dim3((unsigned)((n + DC_RPB - 1) / DC_RPB)), dim3(DC_THREADS), 0, ctx->stream, a);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

extern "C" int mcom_range_check_dest(mcom_ctx *ctx, const uint64_t *d_dest, uint64_t dest0, uint64_t n, uint64_t n_rows, uint32_t *d_seen, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0) return MCOM_OK;
	if (!d_seen || !d_flag || n >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "range_check_dest: bad argument");
	MCOM_LAUNCH(k_dc_check_dest, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, d_dest, dest0, n, n_rows, d_seen, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

extern "C" int mcom_range_decode_reads(mcom_ctx *ctx, const mcom_decode_src *src, uint64_t n, int L, const uint64_t *d_dest, uint64_t dest0,
                                        uint64_t win_first, uint64_t win_count, uint8_t *d_out, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0 || win_count == 0) return MCOM_OK;
	if (!src || !d_out || !d_flag || L < 1 || L > 256 || n >= (1ull << 34) || win_first + win_count < win_first) return mcom_fail(ctx, MCOM_E_ARG, "range_decode_reads: bad argument");
	if (src->d_text && !src->d_line_start) return mcom_fail(ctx, MCOM_E_ARG, "range_decode_reads: a text without its line index");
	if (src->d_cid && (!src->d_ref || !src->d_pos || !src->d_coff)) return mcom_fail(ctx, MCOM_E_ARG, "range_decode_reads: a member table without its reference");
	const uint64_t cap = n < win_count ? n : win_count;
	uint64_t *sel = nullptr;                                               // the count, then the list
	MCOM_HIP(ctx, mcom_dmalloc(&sel, (cap + 1) * 8));
	mcom_dfree_later(ctx, sel);
	MCOM_HIP(ctx, hipMemsetAsync(sel, 0, 8, ctx->stream));
	MCOM_LAUNCH(k_dc_select, dim3(dc_blocks(n)), dim3(DC_THREADS), 0, ctx->stream, d_dest, dest0, n, win_first, win_count, sel + 1, cap, (unsigned long long*)sel, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	DcReads a;
	dc_fill(a, src, n, L, d_dest, dest0, d_out, win_first + win_count, nullptr, d_flag);
	MCOM_LAUNCH(k_dc_reads_sel, dim3((unsigned)((cap + DC_RPB - 1) / DC_RPB)), dim3(DC_THREADS), 0, ctx->stream, a, (const uint64_t*)(sel + 1), (const unsigned long long*)sel, cap, win_first);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}

// ---- consensus agreement (`minicom -a Q[:C]`) ---------------------------------------------------------
// coverage   cov[b] = member reads of the stream set whose window [coff[cid] + pos, + L) holds contig base b.  +1 at the window's first
//            base and -1 behind its last into a cleared array of 64-bit words (wrapping), one exclusive scan (scan.hip) over bases + 1
//            words -- cov[b] is entry b + 1 -- and a pass that narrows to bytes, saturating at 255          (k_dc_cov_mark, k_dc_cov_narrow)
// mask       k_dc_reads' window and line walk with a second LDS row that says "still the window byte": a literal clears it unless it
//            equals the window byte.  Then the flag meets the coverage of its place, and the row leaves as bits, reversed when the
//            direction bit is set: column i in bit i & 7 of byte i >> 3 of mask row dest                                  (k_dc_agree)
__global__ __launch_bounds__(DC_THREADS) void k_dc_cov_mark(const uint32_t *__restrict__ cid, const uint32_t *__restrict__ pos, const uint64_t *__restrict__ coff,
                                                            uint64_t n_contigs, uint64_t n_members, int L, uint64_t bases, unsigned long long *__restrict__ diff,
                                                            uint32_t *__restrict__ flag)
{
	const uint64_t q = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (q >= n_members) return;
	const uint64_t c = cid[q];
	if (c >= n_contigs) { atomicOr(flag, MCOM_DECODE_F_BOUNDS); return; }
	const uint64_t off = coff[c] + pos[q];
	if (off > bases || (uint64_t)L > bases - off) { atomicOr(flag, MCOM_DECODE_F_BOUNDS); return; }
	atomicAdd(diff + off, 1ull);
	atomicAdd(diff + off + (uint64_t)L, ~0ull);                             // diff has bases + 1 words
}

__global__ __launch_bounds__(DC_THREADS) void k_dc_cov_narrow(const uint64_t *__restrict__ e, uint64_t bases, uint8_t *__restrict__ cov)
{
	const uint64_t b = (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x;
	if (b >= bases) return;
	const uint64_t v = e[b + 1];
	cov[b] = v > 255 ? (uint8_t)255 : (uint8_t)v;
}

struct DcAgree {
	DcReads r;                                                              // r.out and r.seen are not used
	const uint8_t *cov; uint64_t cov_bases; uint32_t min_cov;
	uint8_t *mask; uint64_t mask_pitch;
};

__global__ __launch_bounds__(DC_THREADS) void k_dc_agree(const DcAgree b)
{
	__shared__ __align__(16) uint8_t s_row[DC_RPB][DC_PITCH];
	__shared__ __align__(16) uint8_t s_win[DC_RPB][DC_PITCH];               // 1: column p of the window still holds the window's byte
	__shared__ uint64_t s_dest[DC_RPB];
	const DcReads &a = b.r;
	const int g = threadIdx.x / DC_G, lane = threadIdx.x % DC_G;
	const uint64_t m = (uint64_t)blockIdx.x * DC_RPB + g;
	const bool live = m < a.n;
	const int L = a.L;
	uint8_t *win = s_win[g];
	bool have; uint64_t off;
	dc_row_steps<true>(a, m, live, g, lane, s_row[g], win, b.cov_bases, s_dest, have, off);
	const uint64_t d = live ? s_dest[g] : ~0ull;
	// 4. the coverage of every agreeing column's place (off + p < cov_bases: checked in 1)
	if (have && d != ~0ull) for (int p = lane; p < L; p += DC_G) if (win[p] && (uint32_t)b.cov[off + p] < b.min_cov) win[p] = 0;
	__syncthreads();
	if (d == ~0ull) return;
	bool rev = false;
	if (a.dir && (m >> 3) < a.dir_bytes) rev = (a.dir[m >> 3] >> (m & 7)) & 1u;
	// 5. the mask row: a lane assembles whole bytes, (L + 7) / 8 of them, none behind the row
	uint8_t *dst = b.mask + d * b.mask_pitch;
	const int n_bytes = (L + 7) >> 3;
	for (int k = lane; k < n_bytes; k += DC_G) {
		uint32_t x = 0;
#pragma unroll
		for (int j = 0; j < 8; ++j) { const int i = 8 * k + j; if (i < L && win[rev ? L - 1 - i : i]) x |= 1u << j; }
		dst[k] = (uint8_t)x;
	}
}

extern "C" int mcom_agree_coverage(mcom_ctx *ctx, const uint32_t *d_cid, const uint32_t *d_pos, const uint64_t *d_coff, uint64_t n_contigs, uint64_t n_members,
                                    int L, uint64_t ref_bases, uint8_t *d_cov, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || L < 1 || L > 256 || (ref_bases && !d_cov)) return mcom_fail(ctx, MCOM_E_ARG, "agree_coverage: bad argument");
	if (n_members && (!d_cid || !d_pos || !d_coff || n_contigs == 0)) return mcom_fail(ctx, MCOM_E_ARG, "agree_coverage: null pointer");
	if (n_members >= DC_MAX_ITEMS || ref_bases >= DC_MAX_ITEMS) return mcom_fail(ctx, MCOM_E_ARG, "agree_coverage: too many members or bases");
	if (ref_bases == 0 && n_members == 0) return MCOM_OK;
	const uint64_t work = (ref_bases + 1) * 8;
	{
		size_t fr = 0, tot = 0;
		MCOM_HIP(ctx, hipMemGetInfo(&fr, &tot));
		if (work + ((uint64_t)64 << 20) > fr)
			return mcom_fail(ctx, MCOM_E_OVERFLOW, "agree_coverage: %llu bytes of counters for %llu contig bases do not fit the card (%zu bytes free)", (unsigned long long)work, (unsigned long long)ref_bases, fr);
	}
	uint64_t *e = nullptr;
	MCOM_HIP(ctx, mcom_dmalloc(&e, work));
	mcom_dfree_later(ctx, e);
	MCOM_HIP(ctx, hipMemsetAsync(e, 0, work, ctx->stream));
	if (n_members) {
		MCOM_LAUNCH(k_dc_cov_mark, dim3(dc_blocks(n_members)), dim3(DC_THREADS), 0, ctx->stream, d_cid, d_pos, d_coff, n_contigs, n_members, L, ref_bases, (unsigned long long*)e, d_flag);
		MCOM_LAUNCH_CHECK(ctx);
	}
	int rc = mcom_scan64(ctx, e, e, ref_bases + 1, nullptr);
	if (rc) return rc;
	if (ref_bases) {
		MCOM_LAUNCH(k_dc_cov_narrow, dim3(dc_blocks(ref_bases)), dim3(DC_THREADS), 0, ctx->stream, (const uint64_t*)e, ref_bases, d_cov);
		MCOM_LAUNCH_CHECK(ctx);
	}
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

extern "C" int mcom_agree_mask(mcom_ctx *ctx, const mcom_decode_src *src, uint64_t n, int L, const uint64_t *d_dest, uint64_t dest0, uint64_t n_rows,
                                 const uint8_t *d_cov, uint64_t cov_bases, uint32_t min_cov, uint8_t *d_mask, uint64_t mask_pitch, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (n == 0) return MCOM_OK;
	if (!src || !d_mask || !d_flag || L < 1 || L > 256 || n >= (1ull << 34)) return mcom_fail(ctx, MCOM_E_ARG, "agree_mask: bad argument");
	if (min_cov < 1 || min_cov > 255 || mask_pitch < (uint64_t)((L + 7) / 8)) return mcom_fail(ctx, MCOM_E_ARG, "agree_mask: coverage %u (1 .. 255), mask pitch %llu for %d columns", min_cov, (unsigned long long)mask_pitch, L);
	if (src->d_text && !src->d_line_start) return mcom_fail(ctx, MCOM_E_ARG, "agree_mask: a text without its line index");
	if (src->d_cid && (!src->d_ref || !src->d_pos || !src->d_coff || !d_cov)) return mcom_fail(ctx, MCOM_E_ARG, "agree_mask: a member table without its reference or its coverage");
	DcAgree b;
	dc_fill(b.r, src, n, L, d_dest, dest0, nullptr, n_rows, nullptr, d_flag);
	b.cov = d_cov; b.cov_bases = cov_bases; b.min_cov = min_cov; b.mask = d_mask; b.mask_pitch = mask_pitch;
	MCOM_LAUNCH(k_dc_agree, dim3((unsigned)((n + DC_RPB - 1) / DC_RPB)), dim3(DC_THREADS), 0, ctx->stream, b);
	MCOM_LAUNCH_CHECK(ctx);
	return MCOM_OK;
}
