// minicom_amd/csrc/inflate.hip -- gzip members inflated on the GPU: mcom_gzip_walk, mcom_gzip_inflate.
// One workgroup of one wave per member; everything that decides a byte or a status is csrc/inflate_model.hpp, which the host twin
// (host/mcom_gzip_gpu.cpp) compiles as well.  LDS per workgroup: about 5.7 KiB (the model's tables with a first level of 2^10 and 2^8
// 16-bit entries, a batch of 64 tokens with their offsets, the CRC table and 64 chunk CRCs), so the wave slots of a CU, not its LDS,
// bound the members in flight.
//   k_gzip_inflate  per member: lane 0 reads a block header and counts the codes; all lanes fill the first-level tables; then batch by
//                   batch lane 0 decodes up to 64 tokens into LDS and the wave expands them: a prefix sum of the tokens' lengths, the
//                   literals stored by their lanes, a barrier, the matches in token order by all lanes (byte j of a match from
//                   src[j % dist] where dist < len) with a barrier behind each, since the next one may read what this one wrote.
//                   Stored blocks are copied by all lanes.  At the end the CRC-32 of 64 chunks and their tree of combine steps.
// The output is its own window: matches read the member's slot in global memory.
#include "mcom_dev.hpp"
#include "inflate_model.hpp"

using namespace mcom_inflate_model;

namespace {

enum { GZ_THREADS = 64 };
static_assert(GZ_THREADS == BATCH, "a lane per token of a batch");

struct GzLds {
	Tables T;
	uint32_t tok[BATCH], off[BATCH];
	uint32_t crc_table[256], crc_v[GZ_THREADS];
	uint64_t sat;                                                 // where a stored block's bytes begin in the payload
	uint32_t ntok, nbytes, status, last, type, slen;
};
static_assert(sizeof(GzLds) * 16 <= 160 * 1024, "sixteen workgroups per CU at least");

__global__ __launch_bounds__(GZ_THREADS) void k_gzip_inflate(const uint8_t *in, const mcom_gzip_member *mem, uint64_t n_members, uint8_t *outb, uint8_t *status)
{
	__shared__ GzLds S;
	const uint32_t lane = threadIdx.x;
	for (uint32_t k = 0; k < 4; ++k) S.crc_table[4 * lane + k] = mcom_deflate::crc_table_entry(4 * lane + k);
	for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
		const mcom_gzip_member M = mem[m];
		const uint8_t *pay = in + M.in_off;
		uint8_t *out = outb + M.out_off;
		const uint64_t slot = M.isize;
		Bits b;                                                       // lane 0's; the others never read through it
		bits_begin(b, pay, M.in_bytes);
		uint64_t w = 0;                                               // bytes of the member written so far (the same in every lane)
		int st = ST_OK;
		__syncthreads();                                              // the member before is done with the LDS
		for (;;) {
			if (lane == 0) {
				uint32_t last = 0, type = 0, slen = 0;
				int s = block_header(b, S.T, last, type);
				if (!s && type == 0) {
					s = stored_begin(b, slen);
					if (!s && slen > slot - w) s = ST_ROOM;
					S.sat = b.at;
				}
				if (!s && type != 0) s = block_codes(S.T);
				S.status = (uint32_t)s; S.last = last; S.type = type; S.slen = slen;
			}
			__syncthreads();
			st = (int)S.status;
			const uint32_t last = S.last, type = S.type;
			if (st) break;
			if (type == 0) {
				const uint32_t slen = S.slen;
				const uint8_t *src = pay + S.sat;
				for (uint32_t i = lane; i < slen; i += GZ_THREADS) out[w + i] = src[i];
				if (lane == 0) stored_end(b, slen);
				w += slen;
				__syncthreads();
			} else {
				block_fast_clear(S.T, lane, GZ_THREADS);
				__syncthreads();
				block_fast_fill(S.T, lane, GZ_THREADS);
				__syncthreads();
				for (;;) {
					if (lane == 0) {
						uint32_t n = 0, nbyt = 0;
						int s = ST_OK;
						while (n < BATCH) {
							uint32_t tok = 0, nb = 0;
							s = decode_token(b, S.T, w + nbyt, slot - w - nbyt, tok, nb);
							if (s) break;
							S.tok[n++] = tok; nbyt += nb;
						}
						S.ntok = n; S.nbytes = nbyt; S.status = (uint32_t)s;
					}
					__syncthreads();
					const uint32_t ntok = S.ntok, nbytes = S.nbytes;
					st = (int)S.status;
					// the tokens in front of an end code or an error passed every check: they are expanded all the same
					const uint32_t t = lane < ntok ? S.tok[lane] : 0;
					const bool mt = lane < ntok && tok_is_match(t);
					const uint32_t ln = lane < ntok ? (mt ? tok_len(t) : 1u) : 0u;
					uint32_t incl = ln;
					for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
					S.off[lane] = incl - ln;
					if (lane < ntok && !mt) out[w + (incl - ln)] = (uint8_t)t;
					uint64_t mm = __ballot(mt);
					__syncthreads();                                      // literals of this batch are there for its matches
					while (mm) {
						const uint32_t i = (uint32_t)__builtin_ctzll(mm);
						mm &= mm - 1;
						const uint32_t tt = S.tok[i], L = tok_len(tt), D = tok_dist(tt);
						uint8_t *dst = out + w + S.off[i];
						const uint8_t *src = dst - D;
						if (D >= L) { for (uint32_t j = lane; j < L; j += GZ_THREADS) dst[j] = src[j]; }
						else { for (uint32_t j = lane; j < L; j += GZ_THREADS) dst[j] = src[j % D]; }
						__syncthreads();                                  // the next match may read these bytes
					}
					w += nbytes;
					__syncthreads();                                      // the batch is read: lane 0 may write the next one
					if (st) break;
				}
				if (st != ST_EOB) break;
				st = ST_OK;
			}
			if (last) break;
		}
		if (!st) {
			if (lane == 0) S.status = (uint32_t)stream_end(b);
			__syncthreads();
			st = (int)S.status;
		}
		if (!st && w != slot) st = ST_CHECK;
		if (!st) {
			const uint64_t chunk = (slot + GZ_THREADS - 1) / GZ_THREADS;
			const uint64_t cb = (uint64_t)lane * chunk, ce = cb + chunk < slot ? cb + chunk : slot;
			S.crc_v[lane] = cb < ce ? crc_bytes(out + cb, ce - cb, S.crc_table) : 0u;
			for (uint32_t s = 1; s < GZ_THREADS; s <<= 1) {
				__syncthreads();
				if ((lane & (2 * s - 1)) == 0 && (uint64_t)(lane + s) * chunk < slot) {
					const uint64_t rb = (uint64_t)(lane + s) * chunk, re = (uint64_t)(lane + 2 * s) * chunk < slot ? (uint64_t)(lane + 2 * s) * chunk : slot;
					S.crc_v[lane] = mcom_deflate::crc_combine(S.crc_v[lane], S.crc_v[lane + s], (uint32_t)(re - rb));
				}
			}
			__syncthreads();
			if (S.crc_v[0] != M.crc) st = ST_CHECK;
		}
		if (lane == 0) status[m] = (uint8_t)st;
	}
}

}  // namespace

static_assert(MCOM_GZIP_OK == ST_OK && MCOM_GZIP_CORRUPT == ST_CORRUPT && MCOM_GZIP_TRUNCATED == ST_TRUNCATED && MCOM_GZIP_ROOM == ST_ROOM && MCOM_GZIP_CHECK == ST_CHECK, "the model's statuses are the interface's");

static_assert(sizeof(mcom_gzip_member) == sizeof(Member) && offsetof(mcom_gzip_member, in_bytes) == offsetof(Member, in_bytes) && offsetof(mcom_gzip_member, out_off) == offsetof(Member, out_off) &&
              offsetof(mcom_gzip_member, isize) == offsetof(Member, isize) && offsetof(mcom_gzip_member, crc) == offsetof(Member, crc), "the model's member is the interface's");

extern "C" int mcom_gzip_walk(const uint8_t *h_file, uint64_t bytes, mcom_gzip_member *h_members, uint64_t cap, uint64_t *n_members, uint64_t *text_bytes, uint64_t *used)
{
	if (!n_members || !text_bytes || !used || (bytes && !h_file)) return MCOM_E_ARG;
	return walk_members(h_file, bytes, reinterpret_cast<Member*>(h_members), cap, n_members, text_bytes, used) ? MCOM_OK : MCOM_E_ARG;
}

extern "C" int mcom_gzip_inflate(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const mcom_gzip_member *d_members, uint64_t n_members,
                                 uint8_t *d_out, uint64_t out_bytes, uint8_t *d_status, uint64_t *h_bad, uint64_t *h_first_bad)
{
	if (!ctx) return MCOM_E_ARG;
	if (!h_bad || !h_first_bad) return mcom_fail(ctx, MCOM_E_ARG, "gzip_inflate: null pointer");
	*h_bad = 0; *h_first_bad = n_members;
	if (!n_members) return MCOM_OK;
	if (!d_members || !d_status || (in_bytes && !d_in) || (out_bytes && !d_out)) return mcom_fail(ctx, MCOM_E_ARG, "gzip_inflate: null pointer");
	// the table's extents, on a host copy: no kernel is launched over a table that leaves a buffer
	std::vector<mcom_gzip_member> tab;
	std::vector<uint8_t> stat;
	try { tab.resize(n_members); stat.resize(n_members); } catch (const std::bad_alloc &) { return mcom_fail(ctx, MCOM_E_NOMEM, "gzip_inflate: no room for a table of %llu members", (unsigned long long)n_members); }
	MCOM_HIP(ctx, hipMemcpyAsync(tab.data(), d_members, n_members * sizeof(mcom_gzip_member), hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	int why = 0;
	const int64_t off = check_table(reinterpret_cast<const Member*>(tab.data()), n_members, in_bytes, out_bytes, &why);
	if (off >= 0) return mcom_fail(ctx, MCOM_E_ARG, why == 0 ? "gzip_inflate: the payload of member %llu leaves the input" : why == 1 ? "gzip_inflate: the slot of member %llu leaves the output" :
	                               "gzip_inflate: the slot of member %llu begins inside the one before", (unsigned long long)off);
	const uint64_t grid_max = 32ull * (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
	const uint32_t grid = (uint32_t)(n_members < grid_max ? n_members : grid_max);
	MCOM_LAUNCH(k_gzip_inflate, dim3(grid), dim3(GZ_THREADS), 0, ctx->stream, d_in, d_members, n_members, d_out, d_status);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(stat.data(), d_status, n_members, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	uint64_t bad = 0, first = n_members;
	for (uint64_t m = 0; m < n_members; ++m) if (stat[m]) { if (!bad) first = m; ++bad; }
	*h_bad = bad; *h_first_bad = first;
	return MCOM_OK;
}
