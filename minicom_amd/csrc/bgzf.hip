// minicom_amd/csrc/bgzf.hip -- BGZF output on the GPU: mcom_bgzf_bound, mcom_bgzf_encode.
// One workgroup of 256 threads per block of 65280 bytes; everything that decides a byte is csrc/deflate_model.hpp, which the host twin
// (host/mcom_bgzf.cpp) compiles as well.  LDS per workgroup (about 102 KiB, so one workgroup = 4 waves per CU): the block as 64-bit
// words (65296 B), the hash table of 2^13 words (32 KiB; after the parse the same room holds the code construction's scratch and the
// plan), both histograms, the tile's jump and reached arrays, the CRC table and chunk CRCs, and a window of 394 words the bits of 256
// tokens are packed into.  The tokens of a block (at most 65281 words) wait in HBM between the parse and the emission.
//   k_bgzf_blocks   per block: load, chunk CRCs and their tree of combine steps; tile by tile the candidates and match lengths (a lane
//                   per position), the greedy chain by pointer doubling inside the tile (8 rounds) from the entry the tile before left,
//                   tokens and histograms; one lane builds the plan; all lanes pack the tokens' bits (prefix sum of bit lengths,
//                   atomicOr into the zeroed window in LDS, whole words out with plain stores)
//   k_bgzf_offsets  exclusive scan of the members' sizes (one workgroup)
//   k_bgzf_compact  a workgroup per member: header, payload (the staged bits, or the text itself for a stored block), trailer
#include "mcom_dev.hpp"
#include "deflate_model.hpp"

using namespace mcom_deflate;

namespace {

enum { BZ_THREADS = 256, BZ_WIN_WORDS = 394, BZ_STAGE = 65312, BZ_TOK_STRIDE = 65288, BZ_ROUND_BLOCKS = 4096 };
static_assert(BZ_THREADS == TILE, "a lane per position of a tile");
static_assert(sizeof(Work) + sizeof(Plan) + 16 <= HASH_SLOTS * 4, "the plan and its scratch take the hash table's room");
static_assert(BZ_STAGE % 16 == 0 && BZ_STAGE >= BLOCK + STORED_BYTES + 8, "room for every dynamic payload, rounded up to words");

struct BzMeta { uint32_t payload, crc, isize, stored; };

struct BzLds {
	uint64_t text[TEXT_WORDS];
	uint32_t hash[HASH_SLOTS];
	uint32_t ll[288], dd[32];
	uint32_t crc_table[256], crc_v[256];
	uint32_t win[BZ_WIN_WORDS];
	uint32_t wcnt[4];
	uint32_t entry, hbits;
	uint16_t jump[TILE];
	uint8_t reached[TILE];
};

struct LdsPut {                                                   // write_header's sink: bits into the window, one lane
	uint32_t *win; uint32_t at;
	__device__ void operator()(uint32_t v, uint32_t bits)
	{
		if (!bits) return;
		const uint32_t w = at >> 5, s = at & 31;
		win[w] |= v << s;
		if (s + bits > 32) win[w + 1] |= v >> (32 - s);
		at += bits;
	}
};

__global__ __launch_bounds__(BZ_THREADS) void k_bgzf_blocks(const uint8_t *in, uint64_t n, uint32_t nblk, uint32_t *toks_all, uint8_t *stage, BzMeta *meta)
{
	extern __shared__ __align__(16) unsigned char bz_lds[];
	BzLds &S = *reinterpret_cast<BzLds*>(bz_lds);
	Work *work = reinterpret_cast<Work*>(S.hash);
	Plan *plan = reinterpret_cast<Plan*>(reinterpret_cast<unsigned char*>(S.hash) + ((sizeof(Work) + 15) & ~(size_t)15));
	const uint32_t l = threadIdx.x, lane = l & 63, wave = l >> 6;
	uint32_t *toks = toks_all + (size_t)blockIdx.x * BZ_TOK_STRIDE;
	S.crc_table[l] = crc_table_entry(l);
	for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
		const uint64_t off = (uint64_t)blk * BLOCK;
		const uint32_t bn = (uint32_t)(n - off < BLOCK ? n - off : BLOCK);
		__syncthreads();                                          // the block before is done with the LDS
		{	// the text: aligned 64-bit loads, shifted into place; no word is read that holds no byte of the block
			const uintptr_t a0 = (uintptr_t)(in + off);
			const uint32_t sh = (uint32_t)(a0 & 7) * 8;
			const uint64_t *A = reinterpret_cast<const uint64_t*>(a0 & ~(uintptr_t)7);
			const uint32_t nA = (sh / 8 + bn + 7) / 8;
			for (uint32_t w = l; w < TEXT_WORDS; w += BZ_THREADS) {
				uint64_t v = 0;
				if (8 * w < bn) {
					const uint64_t lo = A[w], hi = (sh && w + 1 < nA) ? A[w + 1] : 0;
					v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
					const uint32_t rem = bn - 8 * w;
					if (rem < 8) v &= (1ull << (8 * rem)) - 1;
				}
				S.text[w] = v;
			}
		}
		for (uint32_t i = l; i < HASH_SLOTS; i += BZ_THREADS) S.hash[i] = 0;
		for (uint32_t i = l; i < 288; i += BZ_THREADS) S.ll[i] = 0;
		if (l < 32) S.dd[l] = 0;
		if (l == 0) S.entry = 0;
		__syncthreads();
		// CRC-32: a chunk per lane, joined pairwise
		{
			const uint32_t nch = (bn + CRC_CHUNK - 1) / CRC_CHUNK;
			if (l < nch) { const uint32_t b = l * CRC_CHUNK, e = b + CRC_CHUNK < bn ? b + CRC_CHUNK : bn; S.crc_v[l] = crc_chunk(S.text, b, e, S.crc_table); }
			for (uint32_t s = 1; s < BZ_THREADS; s <<= 1) {
				__syncthreads();
				if ((l & (2 * s - 1)) == 0 && l + s < nch) {
					const uint32_t rb = (l + s) * CRC_CHUNK, re = (l + 2 * s) * CRC_CHUNK < bn ? (l + 2 * s) * CRC_CHUNK : bn;
					S.crc_v[l] = crc_combine(S.crc_v[l], S.crc_v[l + s], re - rb);
				}
			}
			__syncthreads();
		}
		const uint32_t crc = S.crc_v[0];
		// the parse, tile by tile
		uint32_t ntok = 0, entry = 0;
		for (uint32_t base = 0; base < bn; base += TILE) {
			const uint32_t T = bn - base < TILE ? bn - base : TILE, p = base + l;
			const bool valid = l < T;
			Match m = {0, 0};
			uint32_t h = 0; bool hv = false;
			if (valid) {
				hv = p + 4 <= bn;
				uint32_t te = 0;
				if (hv) { h = hash4((uint32_t)load64(S.text, p)); te = S.hash[h]; }
				m = find_match(S.text, bn, p, te);
			}
			const uint32_t step = m.len ? m.len : 1;
			S.jump[l] = valid ? (uint16_t)(l + step) : (uint16_t)0xFFFF;
			S.reached[l] = valid && p == entry;
			__syncthreads();
			for (int r = 0; r < 8; ++r) {                           // after round r the first 2^(r+1) positions of the chain inside the tile are marked
				const uint32_t jj = S.jump[l], rr = S.reached[l];
				const uint32_t j2 = jj < T ? S.jump[jj] : jj;
				__syncthreads();
				if (rr && jj < T) S.reached[jj] = 1;
				S.jump[l] = (uint16_t)j2;
				__syncthreads();
			}
			const bool reached = valid && S.reached[l];
			if (reached && l + step >= T) S.entry = p + step;       // the one position whose token leaves the tile
			const uint64_t ball = __ballot(reached);
			if (lane == 0) S.wcnt[wave] = (uint32_t)__popcll(ball);
			__syncthreads();
			uint32_t before = 0, total = 0;
			for (uint32_t w = 0; w < 4; ++w) { const uint32_t c = S.wcnt[w]; if (w < wave) before += c; total += c; }
			if (reached) {
				const uint32_t at = ntok + before + (uint32_t)__popcll(ball & ((1ull << lane) - 1));
				uint32_t tok;
				if (m.len) {
					uint32_t s, eb, ev;
					len_symbol(m.len, s, eb, ev); atomicAdd(&S.ll[s], 1u);
					dist_symbol(m.dist, s, eb, ev); atomicAdd(&S.dd[s], 1u);
					tok = match_token(m);
				} else {
					tok = (uint32_t)(S.text[p >> 3] >> ((p & 7) * 8)) & 255;
					atomicAdd(&S.ll[tok], 1u);
				}
				if (at < MAX_TOKENS) toks[at] = tok;
			}
			ntok += total;
			if (hv) atomicMax(&S.hash[h], p + 1);
			__syncthreads();
			entry = S.entry;
		}
		if (l == 0) { if (ntok < MAX_TOKENS) toks[ntok] = EOB; S.ll[EOB] = 1; }
		++ntok;
		__syncthreads();                                          // the table is dead: its room becomes the plan's
		if (l == 0) plan_block(S.ll, S.dd, bn, plan, work);
		for (uint32_t i = l; i < BZ_WIN_WORDS; i += BZ_THREADS) S.win[i] = 0;
		__syncthreads();
		if (plan->stored) {
			if (l == 0) { BzMeta mt = {STORED_BYTES + bn, crc, bn, 1u}; meta[blk] = mt; }
			continue;
		}
		uint32_t *out32 = reinterpret_cast<uint32_t*>(stage + (size_t)blk * BZ_STAGE);
		if (l == 0) { LdsPut put = {S.win, 0}; write_header(plan, put); S.hbits = put.at; }
		__syncthreads();
		uint32_t bitpos = S.hbits, wb = 0;                          // bits written so far; the stream's word that win[0] is
		for (uint32_t c = 0; ; c += BZ_THREADS) {
			// whole words out, the open one to the window's front
			const uint32_t nfull = (bitpos >> 5) - wb;
			const uint32_t carry = S.win[nfull];
			for (uint32_t i = l; i < nfull; i += BZ_THREADS) if (wb + i < BZ_STAGE / 4) out32[wb + i] = S.win[i];
			__syncthreads();
			for (uint32_t i = l; i <= nfull + 2 && i < BZ_WIN_WORDS; i += BZ_THREADS) S.win[i] = i == 0 ? carry : 0;
			wb += nfull;
			__syncthreads();
			if (c >= ntok) break;
			uint64_t bits = 0; uint32_t nb = 0;
			if (c + l < ntok) encode_token(plan, toks[c + l], bits, nb);
			uint32_t incl = nb;
			for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
			if (lane == 63) S.wcnt[wave] = incl;
			__syncthreads();
			uint32_t before = 0, total = 0;
			for (uint32_t w = 0; w < 4; ++w) { const uint32_t v = S.wcnt[w]; if (w < wave) before += v; total += v; }
			if (nb) {
				const uint32_t pos = bitpos - 32 * wb + before + incl - nb, w0 = pos >> 5, s = pos & 31;
				const uint64_t lo = bits << s;
				const uint32_t hi = s ? (uint32_t)(bits >> (64 - s)) : 0;
				if (w0 + 2 < BZ_WIN_WORDS) {
					if ((uint32_t)lo) atomicOr(&S.win[w0], (uint32_t)lo);
					if ((uint32_t)(lo >> 32)) atomicOr(&S.win[w0 + 1], (uint32_t)(lo >> 32));
					if (hi) atomicOr(&S.win[w0 + 2], hi);
				}
			}
			bitpos += total;
			__syncthreads();
		}
		if (l == 0) {
			if ((bitpos & 31) && wb < BZ_STAGE / 4) out32[wb] = S.win[0];
			BzMeta mt = {(bitpos + 7) >> 3, crc, bn, 0u}; meta[blk] = mt;
		}
	}
}

// offs[b] = sizes of the members before b; *total = all of them
__global__ __launch_bounds__(BZ_THREADS) void k_bgzf_offsets(const BzMeta *meta, uint32_t nblk, uint64_t *offs, uint64_t *total)
{
	__shared__ uint64_t part[BZ_THREADS];
	const uint32_t l = threadIdx.x, per = (nblk + BZ_THREADS - 1) / BZ_THREADS, b0 = l * per, b1 = b0 + per < nblk ? b0 + per : nblk;
	uint64_t sum = 0;
	for (uint32_t b = b0; b < b1; ++b) sum += HEADER_BYTES + meta[b].payload + TRAILER_BYTES;
	part[l] = sum;
	__syncthreads();
	uint64_t at = 0;
	for (uint32_t i = 0; i < l; ++i) at += part[i];
	for (uint32_t b = b0; b < b1; ++b) { offs[b] = at; at += HEADER_BYTES + meta[b].payload + TRAILER_BYTES; }
	if (l == BZ_THREADS - 1) *total = at;
}

__global__ __launch_bounds__(BZ_THREADS) void k_bgzf_compact(const uint8_t *in, const uint8_t *stage, const BzMeta *meta, const uint64_t *offs, uint32_t nblk,
                                                              uint8_t *out, uint64_t eof_at)
{
	const uint32_t b = blockIdx.x, l = threadIdx.x;
	if (b >= nblk) {                                              // the file's last, empty member
		if (l < EOF_BYTES) out[eof_at + l] = eof_byte(l);
		return;
	}
	const BzMeta mt = meta[b];
	uint8_t *dst = out + offs[b];
	const uint32_t size = HEADER_BYTES + mt.payload + TRAILER_BYTES;
	if (l < HEADER_BYTES) dst[l] = header_byte(l, size);
	uint8_t *pay = dst + HEADER_BYTES;
	if (mt.stored) {
		const uint8_t *src = in + (uint64_t)b * BLOCK;
		const uint32_t n = mt.isize;
		if (l < STORED_BYTES) pay[l] = l == 0 ? 1 : l == 1 ? (uint8_t)n : l == 2 ? (uint8_t)(n >> 8) : l == 3 ? (uint8_t)~n : (uint8_t)(~n >> 8);
		for (uint32_t i = l; i < n; i += BZ_THREADS) pay[STORED_BYTES + i] = src[i];
	} else {
		const uint8_t *src = stage + (size_t)b * BZ_STAGE;
		for (uint32_t i = l; i < mt.payload; i += BZ_THREADS) pay[i] = src[i];
	}
	if (l < 4) pay[mt.payload + l] = (uint8_t)(mt.crc >> (8 * l));
	else if (l < 8) pay[mt.payload + l] = (uint8_t)(mt.isize >> (8 * (l - 4)));
}

struct BzBlocks {                                                 // the call's device blocks, back to the pool on every way out
	mcom_ctx *ctx;
	std::vector<void*> held;
	explicit BzBlocks(mcom_ctx *c) : ctx(c) {}
	~BzBlocks() { for (void *p : held) mcom_dfree(p); }
	template <class T> bool get(T **out, size_t bytes) { void *p = nullptr; if (mcom_dmalloc(&p, bytes) != hipSuccess) return false; held.push_back(p); *out = (T*)p; return true; }
};

}  // namespace

extern "C" uint64_t mcom_bgzf_bound(uint64_t n) { return bound(n); }

extern "C" int mcom_bgzf_encode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *out_len, int flags)
{
	if (!ctx) return MCOM_E_ARG;
	if (!out_len || !d_out || (n && !d_in)) return mcom_fail(ctx, MCOM_E_ARG, "bgzf_encode: null pointer");
	*out_len = 0;
	const bool eof = (flags & MCOM_BGZF_EOF) != 0;
	const uint64_t nblk_all = (n + BLOCK - 1) / BLOCK;
	if (cap < (uint64_t)(HEADER_BYTES + TRAILER_BYTES) * nblk_all + (eof ? EOF_BYTES : 0))
		return mcom_fail(ctx, MCOM_E_OVERFLOW, "bgzf_encode: room for %llu bytes", (unsigned long long)cap);
	const uint32_t round_blocks = (uint32_t)(nblk_all < BZ_ROUND_BLOCKS ? nblk_all : BZ_ROUND_BLOCKS);
	const uint32_t grid_max = (uint32_t)(2 * (ctx->n_cu > 0 ? ctx->n_cu : 256));
	const uint32_t grid_blocks = round_blocks < grid_max ? round_blocks : grid_max;
	BzBlocks B(ctx);
	uint32_t *d_toks = nullptr; uint8_t *d_stage = nullptr; BzMeta *d_meta = nullptr; uint64_t *d_offs = nullptr;
	if (round_blocks && (!B.get(&d_toks, (size_t)grid_blocks * BZ_TOK_STRIDE * 4) || !B.get(&d_stage, (size_t)round_blocks * BZ_STAGE) ||
	                     !B.get(&d_meta, (size_t)round_blocks * sizeof(BzMeta)) || !B.get(&d_offs, ((size_t)round_blocks + 1) * 8)))
		return mcom_fail(ctx, MCOM_E_NOMEM, "bgzf_encode: no room on the card for the staging of %u blocks", round_blocks);
	const size_t lds = sizeof(BzLds);
	if (round_blocks) MCOM_HIP(ctx, hipFuncSetAttribute((const void*)k_bgzf_blocks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	uint64_t at = 0;
	for (uint64_t b0 = 0; b0 < nblk_all; b0 += BZ_ROUND_BLOCKS) {
		const uint32_t nb = (uint32_t)(nblk_all - b0 < BZ_ROUND_BLOCKS ? nblk_all - b0 : BZ_ROUND_BLOCKS);
		const bool last = b0 + nb == nblk_all;
		const uint8_t *src = d_in + b0 * BLOCK;
		const uint64_t src_n = n - b0 * BLOCK;
		MCOM_LAUNCH(k_bgzf_blocks, dim3(nb < grid_blocks ? nb : grid_blocks), dim3(BZ_THREADS), lds, ctx->stream, src, src_n, nb, d_toks, d_stage, d_meta);
		MCOM_LAUNCH_CHECK(ctx);
		MCOM_LAUNCH(k_bgzf_offsets, dim3(1), dim3(BZ_THREADS), 0, ctx->stream, d_meta, nb, d_offs, d_offs + round_blocks);
		MCOM_LAUNCH_CHECK(ctx);
		uint64_t total = 0;
		MCOM_HIP(ctx, mcom_d2h_async(ctx, &total, d_offs + round_blocks, 8));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		const bool with_eof = last && eof;
		if (at + total + (with_eof ? EOF_BYTES : 0) > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "bgzf_encode: room for %llu bytes", (unsigned long long)cap);
		MCOM_LAUNCH(k_bgzf_compact, dim3(nb + (with_eof ? 1 : 0)), dim3(BZ_THREADS), 0, ctx->stream, src, (const uint8_t*)d_stage, (const BzMeta*)d_meta, (const uint64_t*)d_offs, nb,
		            d_out + at, total);
		MCOM_LAUNCH_CHECK(ctx);
		at += total + (with_eof ? EOF_BYTES : 0);
	}
	if (!nblk_all && eof) {
		MCOM_LAUNCH(k_bgzf_compact, dim3(1), dim3(BZ_THREADS), 0, ctx->stream, d_in, (const uint8_t*)nullptr, (const BzMeta*)nullptr, (const uint64_t*)nullptr, 0u, d_out, (uint64_t)0);
		MCOM_LAUNCH_CHECK(ctx);
		at = EOF_BYTES;
	}
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*out_len = at;
	return MCOM_OK;
}
