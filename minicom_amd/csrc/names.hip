// minicom_amd/csrc/names.hip -- read names and '+' lines as `.mcn` members: names cut into tokens, coded against the record before,
// seven streams through the block-sorting coder (format, token rule, op rule, record walk: name_model.hpp; specification and
// cross-check: host/mcom_names.cpp; DESIGN.md sections 3.10 and 3.12).
//
// encode
//   (mcom_decode_line_index)  the 2 n lines of the name text
//   k_name_count    one lane per record: the record and its predecessor tokenised side by side (name_model.hpp's code_record into a
//                   counting sink), what the record adds to every stream as four packed 64-bit counts
//   (mcom_scan64)   four scans: the record's place in every stream
//   k_name_write    the same walk into a writing sink
//   (mcom_bwt_encode x 7, mcom_device_crc32, mcom_rans_encode last: the kind-1 candidate)
// decode
//   (mcom_bwt_decode x 7)
//   k_name_marks    per op: END | TEXT and DELTA | NUM as packed counts; an op above 5 or a last op that is not END raises the flag
//   k_name_bytes64  tlen, and the literal lengths in front of ptext, widened for the scan; k_name_plus: which records hold a literal
//   (mcom_scan64)   ENDs before an op = its record; TEXT / DELTA / NUM ops before it = its place in tlen / delta / num; the scan of
//                   tlen = its place in text; literals before a record and the scan of their lengths = its place in ptext
//   k_name_segstart the op behind the END of record s * recs_per_seg - 1: where segment s begins
//   k_name_newline  a '\n' among the text bytes or the literal bytes raises the flag
//   k_name_walk<0>  one lane per segment, the previous record's token table in LDS (24 x 2 words per lane, lane-interleaved): the
//                   length of every record's two lines
//   (mcom_scan64)   record offsets in the name text; the total must be the header's text_len
//   k_name_walk<1>  the same walk, writing the bytes
//   (mcom_device_crc32)
// Every loop of the walk is bounded by recs_per_seg, 24 tokens and 255 bytes, never by what a stream holds.  Untrusted input (the rule
// of section 3.5): header ranges, member lengths and the embedded members' raw lengths are judged on the host before a launch; the
// counts above are compared on the host between launches; inside the kernels whatever becomes an index is compared with the size of
// what it indexes, a violation raises the flag word and the access is skipped.
//
// kind 2 (section 3.12), a name text against the name text of its mate file:
//   encode          k_name_count / k_name_write with the mate's line index: record r and the mate's name r go through code_record side by
//                   side; mcom_name_encode's member is made first and kept unless the kind-2 member is strictly smaller
//   decode          recs_per_seg is 1, so the scans above give every RECORD its cursors; k_name_walk_mate<0 / 1>, one lane per record,
//                   cuts the mate's name r into tokens as it goes (name_model.hpp's walk_record_mate) and copies matched text tokens from
//                   the mate text: no table, no chain from record to record
//
// FASTQ ends (`minicom -N`): k_fastq_name_lens / k_fastq_name_copy (text -> name text, sixteen lanes per record), k_fastq_emit_named
// (rows and name text -> records), k_name_compare (two name texts, record against record).
#include "mcom_dev.hpp"
#include "name_model.hpp"

using namespace mcom_name;

#define NM_THREADS 256
#define NM_WALK_THREADS 64
#define NM_G 16                                             // lanes per record in the FASTQ kernels

namespace {
struct Blocks {                                             // pooled device blocks of one call, back to the pool once the stream has passed them
	mcom_ctx *ctx; std::vector<void*> v;
	explicit Blocks(mcom_ctx *c) : ctx(c) {}
	~Blocks() { for (void *p : v) mcom_dfree_later(ctx, p); }
	template <class T> hipError_t get(T **out, size_t bytes) { hipError_t e = mcom_dmalloc((void**)out, bytes ? bytes : 16); if (e == hipSuccess) v.push_back(*out); return e; }
};
unsigned blocks_for(uint64_t items, unsigned threads = NM_THREADS) { return (unsigned)((items + threads - 1) / threads); }
unsigned grid_capped(mcom_ctx *ctx, uint64_t items)
{
	const uint64_t g = (items + NM_THREADS - 1) / NM_THREADS, gmax = (uint64_t)(ctx->n_cu > 0 ? ctx->n_cu : 64) * 8;
	return (unsigned)(g > gmax ? gmax : g ? g : 1);
}
}  // namespace

// ---- encode ----------------------------------------------------------------------------------------------------------------------------
// (The bytes of a record's literal are not counted here: a record has at most one, of pl_len bytes, and k_name_count takes that length
// itself from the plus kind code_record returns, behind an optimisation barrier.  Summed in literal(), or selected from pl_len in plain
// sight, the code that hipcc of ROCm 7.2.0 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0) makes for gfx950 at -O3 gave 0 bytes to a '+'
// text that is as long as the name without being the name: the value is set to pl_len before code_record's compare loop and cleared
// behind it for every lane that ran the loop, whatever the loop found, so the member came out without its literal bytes.  DESIGN.md
// section 3.12 has the assembly and a reduced form of the source.  k_name_write runs the same code_record into stores, which cannot be
// folded that way; tests/test_gpu_mate_names.py holds both kernels to the host twin's bytes on exactly such records.  Check the
// barrier again with every new compiler: without it that test fails.)
struct NmCountSink {
	uint32_t ops = 0, n_delta = 0, n_num = 0, n_tlen = 0, n_text = 0, n_lit = 0;
	__device__ void op(uint32_t) { ++ops; }
	__device__ void delta(uint8_t) { ++n_delta; }
	__device__ void num(uint32_t) { ++n_num; }
	__device__ void text(const uint8_t *, uint32_t n) { ++n_tlen; n_text += n; }
	__device__ void plus(uint32_t) {}
	__device__ void literal(const uint8_t *, uint32_t) { ++n_lit; }
};
struct NmWriteSink {
	uint8_t *ops, *deltas, *nums, *tlens, *texts, *plus_at, *lit_len, *lit_bytes;
	__device__ void op(uint32_t b) { *ops++ = (uint8_t)b; }
	__device__ void delta(uint8_t b) { *deltas++ = b; }
	__device__ void num(uint32_t v) { nums[0] = (uint8_t)v; nums[1] = (uint8_t)(v >> 8); nums[2] = (uint8_t)(v >> 16); nums[3] = (uint8_t)(v >> 24); nums += 4; }
	__device__ void text(const uint8_t *p, uint32_t n) { *tlens++ = (uint8_t)n; for (uint32_t j = 0; j < n; ++j) texts[j] = p[j]; texts += n; }
	__device__ void plus(uint32_t b) { *plus_at = (uint8_t)b; }
	__device__ void literal(const uint8_t *p, uint32_t n) { *lit_len = (uint8_t)n; for (uint32_t j = 0; j < n; ++j) lit_bytes[j] = p[j]; }
};
// the three lines a record is coded from; false: one of them is longer than NM_NAME_MAX (the record, or the one after it, is flagged)
struct NmLines { const uint8_t *cur, *prv, *pl; uint32_t clen, plen, pl_len; bool first; };
// mate != NULL (kind 2): the record is coded against line 2 r of the mate text, never against the record before
__device__ __forceinline__ bool nm_lines(const uint8_t *text, const uint64_t *start, uint64_t r, uint32_t rps, const uint8_t *mate, const uint64_t *mstart, NmLines &l)
{
	const uint64_t a = start[2 * r], b = start[2 * r + 1], c = start[2 * r + 2];
	if (!(a < b && b < c) || b - 1 - a > NM_NAME_MAX || c - 1 - b > NM_NAME_MAX) return false;
	l.cur = text + a; l.clen = (uint32_t)(b - 1 - a); l.pl = text + b; l.pl_len = (uint32_t)(c - 1 - b);
	l.first = !mate && r % rps == 0; l.prv = l.cur; l.plen = 0;
	if (mate) {
		const uint64_t p = mstart[2 * r], q = mstart[2 * r + 1];
		if (!(p < q) || q - 1 - p > NM_NAME_MAX) return false;
		l.prv = mate + p; l.plen = (uint32_t)(q - 1 - p);
	} else if (!l.first) {
		const uint64_t p = start[2 * r - 2], q = start[2 * r - 1];
		if (!(p < q) || q - 1 - p > NM_NAME_MAX) return false;
		l.prv = text + p; l.plen = (uint32_t)(q - 1 - p);
	}
	return true;
}

// cnt: four arrays of n + 1 words behind one another: ops << 32 | deltas, nums << 32 | tlens, text bytes << 32 | literal bytes, literals
__global__ __launch_bounds__(NM_THREADS) void k_name_count(const uint8_t *__restrict__ text, uint64_t text_len, const uint64_t *__restrict__ start, uint64_t n, uint32_t rps,
                                                           const uint8_t *__restrict__ mate, const uint64_t *__restrict__ mstart, uint64_t *__restrict__ cnt, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r == 0 && start[2 * n] != text_len) atomicOr(&flag[0], (uint32_t)NM_F_LINES);
	if (r > n) return;
	NmCountSink s;
	uint32_t n_ptext = 0;
	if (r < n) {
		NmLines l;
		const uint64_t a = start[2 * r], b = start[2 * r + 1], c = start[2 * r + 2];
		if (c > text_len || !(a < b && b < c)) atomicOr(&flag[0], (uint32_t)NM_F_LINES);
		else if (b - 1 - a > NM_NAME_MAX || c - 1 - b > NM_NAME_MAX) { atomicOr(&flag[0], (uint32_t)NM_F_LONG); atomicMin(&flag[1], (uint32_t)r); }
		else if (nm_lines(text, start, r, rps, mate, mstart, l)) {
			const uint32_t kind = code_record(l.cur, l.clen, l.prv, l.plen, l.first, l.pl, l.pl_len, s);
			uint32_t pl = l.pl_len;
			asm volatile("" : "+v"(pl));                                          // (see NmCountSink)
			n_ptext = kind == PLUS_LITERAL ? pl : 0u;
		}
	}
	cnt[r] = (uint64_t)s.ops << 32 | s.n_delta;
	cnt[(n + 1) + r] = (uint64_t)s.n_num << 32 | s.n_tlen;
	cnt[2 * (n + 1) + r] = (uint64_t)s.n_text << 32 | n_ptext;
	cnt[3 * (n + 1) + r] = s.n_lit;
}

// off: the scans of cnt.  streams: the seven streams behind one another at base[0 .. 6]; n_lit: literals in all
__global__ __launch_bounds__(NM_THREADS) void k_name_write(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t n, uint32_t rps,
                                                           const uint8_t *__restrict__ mate, const uint64_t *__restrict__ mstart, const uint64_t *__restrict__ off, uint8_t *__restrict__ streams, const uint64_t *__restrict__ base, uint64_t n_lit)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r >= n) return;
	NmLines l;
	if (!nm_lines(text, start, r, rps, mate, mstart, l)) return;                          // (cannot be: the count pass flagged it and nothing is written then)
	const uint64_t a = off[r], b = off[(n + 1) + r], c = off[2 * (n + 1) + r], d = off[3 * (n + 1) + r];
	NmWriteSink s;
	s.ops = streams + base[S_OPS] + (a >> 32); s.deltas = streams + base[S_DELTA] + (a & 0xFFFFFFFFu);
	s.nums = streams + base[S_NUM] + 4 * (b >> 32); s.tlens = streams + base[S_TLEN] + (b & 0xFFFFFFFFu);
	s.texts = streams + base[S_TEXT] + (c >> 32);
	s.plus_at = streams + base[S_PLUS] + r;
	s.lit_len = streams + base[S_PTEXT] + d; s.lit_bytes = streams + base[S_PTEXT] + n_lit + (c & 0xFFFFFFFFu);
	code_record(l.cur, l.clen, l.prv, l.plen, l.first, l.pl, l.pl_len, s);
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------------
// a[i] = END << 32 | TEXT, b[i] = DELTA << 32 | NUM of op i; a[m] = b[m] = 0, so that the exclusive scans end with the totals
__global__ __launch_bounds__(NM_THREADS) void k_name_marks(const uint8_t *__restrict__ ops, uint64_t m, uint64_t *__restrict__ a, uint64_t *__restrict__ b, uint32_t *__restrict__ flag)
{
	const uint64_t i = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (i > m) return;
	uint64_t va = 0, vb = 0;
	if (i < m) {
		const uint32_t v = ops[i];
		if (v > OP_END || (i == m - 1 && v != OP_END)) atomicOr(flag, (uint32_t)NM_F_OP);
		va = v == OP_END ? (uint64_t)1 << 32 : v == OP_TEXT ? 1u : 0u;
		vb = v == OP_DELTA ? (uint64_t)1 << 32 : v == OP_NUM ? 1u : 0u;
	}
	a[i] = va; b[i] = vb;
}
__global__ __launch_bounds__(NM_THREADS) void k_name_bytes64(const uint8_t *__restrict__ src, uint64_t n, uint64_t *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (i > n) return;
	out[i] = i < n ? (uint64_t)src[i] : 0ull;
}
__global__ __launch_bounds__(NM_THREADS) void k_name_plus(const uint8_t *__restrict__ plus, uint64_t n, uint64_t *__restrict__ out, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r > n) return;
	uint64_t v = 0;
	if (r < n) { const uint32_t k = plus[r]; if (k > PLUS_LITERAL) atomicOr(flag, (uint32_t)NM_F_OP); v = k == PLUS_LITERAL; }
	out[r] = v;
}
__global__ __launch_bounds__(NM_THREADS) void k_name_newline(const uint8_t *__restrict__ p, uint64_t n, uint32_t *__restrict__ flag)
{
	bool hit = false;
	for (uint64_t i = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NM_THREADS) hit |= p[i] == '\n';
	if (hit) atomicOr(flag, (uint32_t)NM_F_NL);
}
// seg_op[s] = the op behind the END that closes record s * rps - 1 (seg_op[0] = 0); a: the scan of k_name_marks' first array
__global__ __launch_bounds__(NM_THREADS) void k_name_segstart(const uint8_t *__restrict__ ops, uint64_t m, const uint64_t *__restrict__ a, uint32_t rps, uint64_t n_seg, uint64_t *__restrict__ seg_op)
{
	const uint64_t i = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (i == 0) seg_op[0] = 0;
	if (i >= m || ops[i] != OP_END) return;
	const uint64_t e = (a[i] >> 32) + 1;
	if (e % rps == 0 && e / rps < n_seg) seg_op[e / rps] = i + 1;
}

struct NmLdsTab {
	uint32_t *v, *l;
	__device__ __forceinline__ uint32_t &val(uint32_t t) { return v[t * NM_WALK_THREADS]; }
	__device__ __forceinline__ uint32_t &len(uint32_t t) { return l[t * NM_WALK_THREADS]; }
};
struct NmDecodeArgs {
	View v;
	const uint8_t *plus, *ptext; uint64_t n_ptext, n_lit;                  // ptext: n_lit lengths, then the literal bytes
	const uint64_t *sa, *sb, *st, *sp, *sl;                                 // scans: marks a, marks b, tlen, literal flags, literal lengths
	const uint64_t *seg_op;
	uint64_t n, n_seg, text_len; uint32_t rps;
};
// WRITE = 0: rec[r] = bytes of record r in the name text (0 behind a refused record: rec is cleared before).  WRITE = 1: rec = the scan
// of those, out = the name text.
template <int WRITE>
__global__ __launch_bounds__(NM_WALK_THREADS) void k_name_walk(NmDecodeArgs A, uint64_t *__restrict__ rec, uint8_t *__restrict__ out, uint32_t *__restrict__ flag)
{
	__shared__ uint32_t s_val[TOKEN_CAP * NM_WALK_THREADS], s_len[TOKEN_CAP * NM_WALK_THREADS];
	const uint64_t seg = (uint64_t)blockIdx.x * NM_WALK_THREADS + threadIdx.x;
	if (seg >= A.n_seg) return;
	NmLdsTab tab = { s_val + threadIdx.x, s_len + threadIdx.x };
	Cursor c;
	c.op = A.seg_op[seg];
	if (c.op > A.v.n_ops) { atomicOr(flag, (uint32_t)NM_F_RUN); return; }
	c.tlen = A.sa[c.op] & 0xFFFFFFFFu; c.delta = A.sb[c.op] >> 32; c.num = A.sb[c.op] & 0xFFFFFFFFu;
	if (c.tlen > A.v.n_tlen || c.delta > A.v.n_delta || c.num > A.v.n_num) { atomicOr(flag, (uint32_t)NM_F_RUN); return; }
	c.text = A.st[c.tlen];
	const uint64_t r0 = seg * A.rps, r1 = r0 + A.rps < A.n ? r0 + A.rps : A.n;
	uint64_t lit = A.sp[r0];
	if (lit > A.n_lit) { atomicOr(flag, (uint32_t)NM_F_RUN); return; }
	uint64_t lit_at = A.n_lit + A.sl[lit];
	uint32_t n_prev = 0, bad = 0;
	for (uint64_t r = r0; r < r1 && !bad; ++r) {
		uint8_t *o = nullptr; uint32_t room = NM_NAME_MAX, have = 0;
		if (WRITE) {
			const uint64_t at = rec[r], end = rec[r + 1];
			if (end < at || end > A.text_len || end - at < 2) { bad = NM_F_RUN; break; }
			o = out + at; have = (uint32_t)(end - at < 2 * NM_NAME_MAX + 2 ? end - at : 2 * NM_NAME_MAX + 2) - 2;        // bytes of the two lines without their newlines
			room = have < NM_NAME_MAX ? have : NM_NAME_MAX;
		}
		uint32_t nl = 0;
		bad = walk_record(A.v, c, tab, n_prev, o, room, nl);     // (with WRITE the record's own room, known from the first walk, bounds the name)
		if (bad) break;
		const uint32_t kind = A.plus[r];
		uint32_t pl = 0;
		if (kind == PLUS_NAME) pl = nl;
		else if (kind == PLUS_LITERAL) {
			if (lit >= A.n_lit) { bad = NM_F_RUN; break; }
			pl = A.ptext[lit];
			if (lit_at + pl > A.n_ptext) { bad = NM_F_RUN; break; }
		} else if (kind != PLUS_BARE) { bad = NM_F_OP; break; }
		if (WRITE) {
			if (nl + pl != have) { bad = NM_F_RUN; break; }                 // (cannot be: the first walk measured this record)
			o[nl] = '\n';
			uint8_t *q = o + nl + 1;
			if (kind == PLUS_NAME) for (uint32_t j = 0; j < nl; ++j) q[j] = o[j];
			else if (kind == PLUS_LITERAL) for (uint32_t j = 0; j < pl; ++j) q[j] = A.ptext[lit_at + j];
			q[pl] = '\n';
		} else rec[r] = (uint64_t)nl + pl + 2;
		if (kind == PLUS_LITERAL) { ++lit; lit_at += pl; }
	}
	if (bad) atomicOr(flag, bad);
}

// Kind 2: one lane per record.  A record's cursors are what k_name_walk reads for a segment (recs_per_seg is 1: seg_op[r] is record r's
// first op); its mate name is line 2 r of the mate text (mstart: the mate's line index, checked by k_name_lines before the launch).
// WRITE as above.  A refused record reads nothing outside the streams and the mate text and writes at most its own room.
template <int WRITE>
__global__ __launch_bounds__(NM_THREADS) void k_name_walk_mate(NmDecodeArgs A, const uint8_t *__restrict__ mate, uint64_t mate_len, const uint64_t *__restrict__ mstart,
                                                               uint64_t *__restrict__ rec, uint8_t *__restrict__ out, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r >= A.n) return;
	uint32_t bad = 0;
	do {
		const uint64_t ma = mstart[2 * r], mb = mstart[2 * r + 1];
		if (!(ma < mb) || mb > mate_len || mb - 1 - ma > NM_NAME_MAX) { bad = NM_F_MATE; break; }
		Cursor c;
		c.op = A.seg_op[r];
		if (c.op > A.v.n_ops) { bad = NM_F_RUN; break; }
		c.tlen = A.sa[c.op] & 0xFFFFFFFFu; c.delta = A.sb[c.op] >> 32; c.num = A.sb[c.op] & 0xFFFFFFFFu;
		if (c.tlen > A.v.n_tlen || c.delta > A.v.n_delta || c.num > A.v.n_num) { bad = NM_F_RUN; break; }
		c.text = A.st[c.tlen];
		const uint64_t lit = A.sp[r];
		if (lit > A.n_lit) { bad = NM_F_RUN; break; }
		const uint64_t lit_at = A.n_lit + A.sl[lit];
		uint8_t *o = nullptr; uint32_t room = NM_NAME_MAX, have = 0;
		if (WRITE) {
			const uint64_t at = rec[r], end = rec[r + 1];
			if (end < at || end > A.text_len || end - at < 2) { bad = NM_F_RUN; break; }
			o = out + at; have = (uint32_t)(end - at < 2 * NM_NAME_MAX + 2 ? end - at : 2 * NM_NAME_MAX + 2) - 2;
			room = have < NM_NAME_MAX ? have : NM_NAME_MAX;
		}
		uint32_t nl = 0;
		if ((bad = walk_record_mate(A.v, c, mate + ma, (uint32_t)(mb - 1 - ma), o, room, nl))) break;
		const uint32_t kind = A.plus[r];
		uint32_t pl = 0;
		if (kind == PLUS_NAME) pl = nl;
		else if (kind == PLUS_LITERAL) {
			if (lit >= A.n_lit) { bad = NM_F_RUN; break; }
			pl = A.ptext[lit];
			if (lit_at + pl > A.n_ptext) { bad = NM_F_RUN; break; }
		} else if (kind != PLUS_BARE) { bad = NM_F_OP; break; }
		if (WRITE) {
			if (nl + pl != have) { bad = NM_F_RUN; break; }                     // (cannot be: the first walk measured this record)
			o[nl] = '\n';
			uint8_t *q = o + nl + 1;
			if (kind == PLUS_NAME) for (uint32_t j = 0; j < nl; ++j) q[j] = o[j];
			else if (kind == PLUS_LITERAL) for (uint32_t j = 0; j < pl; ++j) q[j] = A.ptext[lit_at + j];
			q[pl] = '\n';
		} else rec[r] = (uint64_t)nl + pl + 2;
	} while (0);
	if (bad) atomicOr(flag, bad);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
extern "C" uint64_t mcom_name_bound(uint64_t text_len) { return bound(text_len); }

extern "C" int mcom_name_info(const uint8_t *h_member_prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len)
{
	NHeader hd;
	if (!h_member_prefix || !n_records || !text_len || !read_nfields(h_member_prefix, len, hd)) return -1;
	*n_records = hd.n_records; *text_len = hd.text_len;
	return 0;
}

// The seven streams of a name text of n > 0 records as `.bwt` members behind one another: *coded (a block of B), *coded_len bytes, their
// lengths in hd.len.  d_mate NULL: every record against the one before it (hd.rps records a segment); otherwise against line 2 r of the
// mate text, whose line index mstart the caller has checked.
static int name_streams(mcom_ctx *ctx, Blocks &B, const uint8_t *d_text, uint64_t text_len, uint64_t n, const uint8_t *d_mate, const uint64_t *mstart, NHeader &hd,
                        uint8_t **coded_out, uint64_t *coded_len, uint64_t *bad_record)
{
	int rc;
	// the lines, and what every record adds to every stream
	uint64_t *start = nullptr, *cnt = nullptr; uint32_t *d_flag = nullptr;
	MCOM_HIP(ctx, B.get(&start, (2 * n + 1) * 8));
	MCOM_HIP(ctx, B.get(&cnt, 4 * (n + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_flag, 16));
	{
		const uint32_t init[4] = {0, 0xFFFFFFFFu, 0, 0};                     // encoder bits | lowest flagged record | the line index's word
		MCOM_HIP(ctx, hipMemcpyAsync(d_flag, init, 16, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
	}
	uint64_t lines = 0;
	if ((rc = mcom_decode_line_index(ctx, d_text, text_len, nullptr, 0, &lines, nullptr))) return rc;
	if (lines != 2 * n) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: %llu lines, not the two lines of each of %llu records", (unsigned long long)lines, (unsigned long long)n);
	if ((rc = mcom_decode_line_index(ctx, d_text, text_len, start, 2 * n, &lines, d_flag + 2))) return rc;
	MCOM_LAUNCH(k_name_count, dim3(blocks_for(n + 1)), dim3(NM_THREADS), 0, ctx->stream, d_text, text_len, (const uint64_t*)start, n, hd.rps, d_mate, mstart, cnt, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	for (int k = 0; k < 4; ++k) if ((rc = mcom_scan64(ctx, cnt + k * (n + 1), cnt + k * (n + 1), n + 1, nullptr))) return rc;
	uint64_t tot[4]; uint32_t flag[4];
	for (int k = 0; k < 4; ++k) MCOM_HIP(ctx, hipMemcpyAsync(&tot[k], cnt + k * (n + 1) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(flag, d_flag, 16, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag[0] & NM_F_LONG) {
		if (bad_record) *bad_record = flag[1];
		return mcom_fail(ctx, MCOM_E_ARG, "name_encode: record %llu has a name or a '+' text above 255 bytes", (unsigned long long)flag[1] + 1);
	}
	if (flag[0] || flag[2]) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: the name text is not %llu complete lines (flag 0x%x)", (unsigned long long)(2 * n), flag[0]);
	const uint64_t n_lit = tot[3];
	uint64_t raw[N_STREAMS], base[N_STREAMS], room = 0, all = 0;
	raw[S_OPS] = tot[0] >> 32; raw[S_DELTA] = tot[0] & 0xFFFFFFFFu; raw[S_NUM] = 4 * (tot[1] >> 32); raw[S_TLEN] = tot[1] & 0xFFFFFFFFu;
	raw[S_TEXT] = tot[2] >> 32; raw[S_PLUS] = n; raw[S_PTEXT] = n_lit + (tot[2] & 0xFFFFFFFFu);
	for (int k = 0; k < N_STREAMS; ++k) {
		if (raw[k] > mcom_bwt::RAW_MAX) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: stream %d takes %llu bytes (a stream is one .bwt member below 4 GiB; larger name texts are not split)", k, (unsigned long long)raw[k]);
		base[k] = all; all += (raw[k] + 15) & ~(uint64_t)15;
		if (raw[k]) room += mcom_bwt_bound(raw[k]);
	}
	uint8_t *streams = nullptr, *coded = nullptr; uint64_t *d_base = nullptr;
	MCOM_HIP(ctx, B.get(&streams, all));
	MCOM_HIP(ctx, B.get(&d_base, sizeof base));
	MCOM_HIP(ctx, hipMemcpyAsync(d_base, base, sizeof base, hipMemcpyHostToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));                                    // (base lives on this frame)
	MCOM_LAUNCH(k_name_write, dim3(blocks_for(n)), dim3(NM_THREADS), 0, ctx->stream, d_text, (const uint64_t*)start, n, hd.rps, d_mate, mstart, (const uint64_t*)cnt, streams, (const uint64_t*)d_base, n_lit);
	MCOM_LAUNCH_CHECK(ctx);
	// the seven members, back to back as the member holds them
	MCOM_HIP(ctx, B.get(&coded, room));
	uint64_t at = 0;
	for (int k = 0; k < N_STREAMS; ++k) {
		hd.len[k] = 0;
		if (!raw[k]) continue;
		uint64_t got = 0;
		if ((rc = mcom_bwt_encode(ctx, streams + base[k], raw[k], coded + at, room - at, &got))) return rc;
		hd.len[k] = got; at += got;
	}
	*coded_out = coded; *coded_len = at;
	return MCOM_OK;
}

extern "C" int mcom_name_info_mate(const uint8_t *h_member_prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len)
{
	NHeader hd;
	if (!h_member_prefix || !n_records || !text_len || !read_nfields(h_member_prefix, len, hd, true)) return -1;
	*n_records = hd.n_records; *text_len = hd.text_len;
	return 0;
}

extern "C" int mcom_name_encode(mcom_ctx *ctx, const uint8_t *d_text, uint64_t text_len, uint64_t n, uint8_t *d_out, uint64_t cap, uint64_t *out_len, uint64_t *bad_record)
{
	if (!ctx) return MCOM_E_ARG;
	if (bad_record) *bad_record = ~(uint64_t)0;
	if (!out_len || !d_out || (text_len && !d_text)) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: null pointer");
	*out_len = 0;
	if (n > N_MAX || text_len > TEXT_MAX) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: %llu records, %llu bytes of name text (at most %llu records; a text below 4 GiB: larger ones are not split)",
	                                                     (unsigned long long)n, (unsigned long long)text_len, (unsigned long long)N_MAX);
	if (text_len < 2 * n || (n == 0 && text_len)) return mcom_fail(ctx, MCOM_E_ARG, "name_encode: %llu bytes are not the two lines of each of %llu records", (unsigned long long)text_len, (unsigned long long)n);
	if (cap < NHEADER_BYTES) return mcom_fail(ctx, MCOM_E_OVERFLOW, "name_encode: room for %llu bytes", (unsigned long long)cap);
	NHeader hd; hd.n_records = n; hd.text_len = text_len;
	uint8_t head[NHEADER_BYTES];
	if (n == 0) {
		write_nheader(head, hd);
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, NHEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		*out_len = NHEADER_BYTES;
		return MCOM_OK;
	}
	Blocks B(ctx);
	int rc;
	uint8_t *coded = nullptr; uint64_t at = 0;
	if ((rc = name_streams(ctx, B, d_text, text_len, n, nullptr, nullptr, hd, &coded, &at, bad_record))) return rc;
	if ((rc = mcom_device_crc32(ctx, d_text, text_len, &hd.crc))) return rc;
	uint64_t total = NHEADER_BYTES + at;
	// kind 1, made last: the `.rans` member of the name text
	uint8_t *d_rans = nullptr; uint64_t rans_len = 0;
	MCOM_HIP(ctx, B.get(&d_rans, mcom_rans::HEADER_BYTES + text_len));
	if ((rc = mcom_rans_encode(ctx, d_text, text_len, d_rans, mcom_rans::HEADER_BYTES + text_len, &rans_len, 0))) return rc;
	const uint8_t *body = coded; uint64_t body_len = at;
	if (NHEADER_BYTES + rans_len < total) {
		NHeader rh; rh.kind = KIND_RANS; rh.n_records = n; rh.text_len = text_len; rh.crc = hd.crc;
		hd = rh; body = d_rans; body_len = rans_len; total = NHEADER_BYTES + rans_len;
	}
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "name_encode: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	write_nheader(head, hd);
	MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, NHEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(d_out + NHEADER_BYTES, body, body_len, hipMemcpyDeviceToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*out_len = total;
	return MCOM_OK;
}

// the 2 n lines of a mate text, checked: its line index in *mstart (a block of B).  MCOM_E_ARG when the text is not 2 n complete lines of at
// most 255 bytes each
static int mate_lines(mcom_ctx *ctx, Blocks &B, const char *who, const uint8_t *d_mate, uint64_t mate_len, uint64_t n, uint64_t **mstart);

extern "C" int mcom_name_encode_mate(mcom_ctx *ctx, const uint8_t *d_text, uint64_t text_len, uint64_t n, const uint8_t *d_mate, uint64_t mate_len, uint8_t *d_out, uint64_t cap,
                                     uint64_t *out_len, uint64_t *bad_record)
{
	if (!ctx) return MCOM_E_ARG;
	uint64_t ind_len = 0;
	int rc = mcom_name_encode(ctx, d_text, text_len, n, d_out, cap, &ind_len, bad_record);      // the member without a mate: kept unless kind 2 is strictly smaller
	if (rc) return rc;
	*out_len = 0;
	if (mate_len && !d_mate) return mcom_fail(ctx, MCOM_E_ARG, "name_encode_mate: null pointer");
	if (mate_len > TEXT_MAX || mate_len < 2 * n || (n == 0 && mate_len)) return mcom_fail(ctx, MCOM_E_ARG, "name_encode_mate: %llu bytes of mate text are not the two lines of each of %llu records", (unsigned long long)mate_len, (unsigned long long)n);
	if (n == 0) { *out_len = ind_len; return MCOM_OK; }
	Blocks B(ctx);
	uint64_t *mstart = nullptr;
	if ((rc = mate_lines(ctx, B, "name_encode_mate", d_mate, mate_len, n, &mstart))) return rc;
	NHeader hd; hd.kind = KIND_MATE; hd.rps = 1; hd.n_records = n; hd.text_len = text_len;
	uint8_t *coded = nullptr; uint64_t at = 0;
	if ((rc = name_streams(ctx, B, d_text, text_len, n, d_mate, (const uint64_t*)mstart, hd, &coded, &at, bad_record))) return rc;
	if (NHEADER_BYTES + at < ind_len) {
		if ((rc = mcom_device_crc32(ctx, d_text, text_len, &hd.crc)) || (rc = mcom_device_crc32(ctx, d_mate, mate_len, &hd.mate_crc))) return rc;
		uint8_t head[NHEADER_BYTES];
		write_nheader(head, hd);
		MCOM_HIP(ctx, hipMemcpyAsync(d_out, head, NHEADER_BYTES, hipMemcpyHostToDevice, ctx->stream));
		MCOM_HIP(ctx, hipMemcpyAsync(d_out + NHEADER_BYTES, coded, at, hipMemcpyDeviceToDevice, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		ind_len = NHEADER_BYTES + at;
	}
	*out_len = ind_len;
	return MCOM_OK;
}

// the lines of a name text that came out of an embedded `.rans` member: 2 n of them, complete, none above NM_NAME_MAX; rec_off[r] = start[2 r]
__global__ __launch_bounds__(NM_THREADS) void k_name_lines(const uint64_t *__restrict__ start, uint64_t n, uint64_t text_len, uint64_t *__restrict__ rec_off, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r > n) return;
	if (r == n) { if (start[2 * n] != text_len) atomicOr(flag, (uint32_t)NM_F_LINES); if (rec_off) rec_off[n] = text_len; return; }
	const uint64_t a = start[2 * r], b = start[2 * r + 1], c = start[2 * r + 2];
	if (!(a < b && b < c) || b - 1 - a > NM_NAME_MAX || c - 1 - b > NM_NAME_MAX) atomicOr(flag, (uint32_t)NM_F_LONG);
	if (rec_off) rec_off[r] = a;
}

static int mate_lines(mcom_ctx *ctx, Blocks &B, const char *who, const uint8_t *d_mate, uint64_t mate_len, uint64_t n, uint64_t **mstart)
{
	int rc;
	uint64_t lines = 0; uint32_t *d_flag = nullptr, flag[2] = {0, 0};
	if ((rc = mcom_decode_line_index(ctx, d_mate, mate_len, nullptr, 0, &lines, nullptr))) return rc;
	if (lines != 2 * n) return mcom_fail(ctx, MCOM_E_ARG, "%s: the mate text has %llu lines, not the two lines of each of %llu records (flag 0x%x)", who, (unsigned long long)lines, (unsigned long long)n, (uint32_t)NM_F_MATE);
	MCOM_HIP(ctx, B.get(mstart, (2 * n + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_flag, 8));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
	if ((rc = mcom_decode_line_index(ctx, d_mate, mate_len, *mstart, 2 * n, &lines, d_flag + 1))) return rc;
	MCOM_LAUNCH(k_name_lines, dim3(blocks_for(n + 1)), dim3(NM_THREADS), 0, ctx->stream, (const uint64_t*)*mstart, n, mate_len, (uint64_t*)nullptr, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(flag, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag[0] || flag[1]) return mcom_fail(ctx, MCOM_E_ARG, "%s: the mate text is not two complete lines of at most 255 bytes per record (flag 0x%x)", who, (uint32_t)NM_F_MATE);
	return MCOM_OK;
}

// with_mate: the caller holds a mate text (mcom_name_decode_mate): kind 2 is taken and decoded against it; kinds 0 and 1 do not look at it
static int name_decode_impl(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, bool with_mate, const uint8_t *d_mate, uint64_t mate_len, uint8_t *d_text, uint64_t cap, uint64_t *text_len,
                            uint64_t *n_records, uint64_t *d_rec_off)
{
	if (!ctx) return MCOM_E_ARG;
	if (!text_len || !n_records || (in_len && !d_in) || (with_mate && mate_len && !d_mate)) return mcom_fail(ctx, MCOM_E_ARG, "name_decode: null pointer");
	*text_len = 0; *n_records = 0;
	if (in_len < NHEADER_BYTES) return mcom_fail(ctx, MCOM_E_ARG, "name_decode: not a .mcn member (%llu bytes)", (unsigned long long)in_len);
	Blocks B(ctx);
	uint8_t hb[NHEADER_BYTES + mcom_rans::HEADER_BYTES] = {0};
	const size_t head_bytes = in_len < sizeof hb ? (size_t)in_len : sizeof hb;
	MCOM_HIP(ctx, hipMemcpyAsync(hb, d_in, head_bytes, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	NHeader hd;
	if (!read_nheader(hb, in_len, hd, with_mate)) return mcom_fail(ctx, MCOM_E_ARG, "name_decode: the header does not describe this member");
	*text_len = hd.text_len; *n_records = hd.n_records;
	if (hd.text_len > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "name_decode: %llu bytes of name text, room for %llu", (unsigned long long)hd.text_len, (unsigned long long)cap);
	auto refuse = [&](const char *why, uint32_t flag = 0) { *text_len = 0; *n_records = 0; return mcom_fail(ctx, MCOM_E_ARG, "name_decode: %s (flag 0x%x)", why, flag); };
	if (hd.text_len && !d_text) return refuse("null pointer");
	const uint64_t n = hd.n_records, n_seg = hd.n_seg();
	int rc;
	uint32_t *d_flag = nullptr, flag = 0;
	MCOM_HIP(ctx, B.get(&d_flag, 16));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 16, ctx->stream));
	uint64_t *mstart = nullptr;
	if (hd.kind == KIND_MATE) {                                            // the mate: the 2 n lines the member was coded against
		uint32_t mcrc = 0;
		if (mate_len > TEXT_MAX || mate_len < 2 * n || (n == 0 && mate_len)) return refuse("the mate text is not the two lines of each of the member's records", NM_F_MATE);
		if (n && (rc = mate_lines(ctx, B, "name_decode", d_mate, mate_len, n, &mstart))) { *text_len = 0; *n_records = 0; return rc; }
		if (mate_len && (rc = mcom_device_crc32(ctx, d_mate, mate_len, &mcrc))) { *text_len = 0; *n_records = 0; return rc; }
		if (mcrc != hd.mate_crc) return refuse("the mate text is not the one the member was coded against", NM_F_MATE);
	}
	if (n == 0) { if (d_rec_off) MCOM_HIP(ctx, hipMemsetAsync(d_rec_off, 0, 8, ctx->stream)); MCOM_HIP(ctx, mcom_stream_sync(ctx)); return MCOM_OK; }
	if (hd.kind == KIND_RANS) {
		uint64_t got = 0, lines = 0;
		if ((rc = mcom_rans_decode(ctx, d_in + NHEADER_BYTES, in_len - NHEADER_BYTES, d_text, hd.text_len, &got)) || got != hd.text_len) { *text_len = 0; *n_records = 0; return rc ? rc : refuse("embedded length"); }
		// (the embedded member's CRC is the header's and was checked.)  The text must still be 2 n lines of at most 255 bytes.
		if ((rc = mcom_decode_line_index(ctx, d_text, hd.text_len, nullptr, 0, &lines, nullptr))) { *text_len = 0; *n_records = 0; return rc; }
		if (lines != 2 * n) return refuse("the text is not two lines per record");
		uint64_t *start = nullptr;
		MCOM_HIP(ctx, B.get(&start, (2 * n + 1) * 8));
		if ((rc = mcom_decode_line_index(ctx, d_text, hd.text_len, start, 2 * n, &lines, d_flag + 1))) { *text_len = 0; *n_records = 0; return rc; }
		MCOM_LAUNCH(k_name_lines, dim3(blocks_for(n + 1)), dim3(NM_THREADS), 0, ctx->stream, (const uint64_t*)start, n, hd.text_len, d_rec_off, d_flag);
		MCOM_LAUNCH_CHECK(ctx);
		uint32_t f2[2] = {0, 0};
		MCOM_HIP(ctx, hipMemcpyAsync(f2, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		if (f2[0] || f2[1]) return refuse("the text is not two lines of at most 255 bytes per record", f2[0]);
		return MCOM_OK;
	}
	// the seven embedded members: their own headers first, then the streams
	uint64_t raw[N_STREAMS] = {0}, m_at[N_STREAMS], s_at[N_STREAMS], all = 0;
	{
		uint8_t heads[N_STREAMS][mcom_bwt::HEADER_BYTES];
		uint64_t at = NHEADER_BYTES;
		for (int k = 0; k < N_STREAMS; ++k) { m_at[k] = at; at += hd.len[k]; if (hd.len[k]) MCOM_HIP(ctx, hipMemcpyAsync(heads[k], d_in + m_at[k], mcom_bwt::HEADER_BYTES, hipMemcpyDeviceToHost, ctx->stream)); }
		MCOM_HIP(ctx, mcom_stream_sync(ctx));
		for (int k = 0; k < N_STREAMS; ++k) if (hd.len[k] && !embedded_raw_len(heads[k], hd.len[k], raw[k])) return refuse("an embedded member's header does not describe it");
	}
	if (!check_raw_lens(hd, raw)) return refuse("the streams' lengths do not fit the header's counts");
	for (int k = 0; k < N_STREAMS; ++k) { s_at[k] = all; all += (raw[k] + 15) & ~(uint64_t)15; }
	uint8_t *streams = nullptr;
	MCOM_HIP(ctx, B.get(&streams, all));
	for (int k = 0; k < N_STREAMS; ++k) {
		if (!raw[k]) continue;
		uint64_t got = 0;
		if ((rc = mcom_bwt_decode(ctx, d_in + m_at[k], hd.len[k], streams + s_at[k], raw[k], &got)) || got != raw[k]) { *text_len = 0; *n_records = 0; return rc ? rc : refuse("embedded length"); }
	}
	const uint64_t m = raw[S_OPS], T = raw[S_TLEN];
	const uint8_t *ops = streams + s_at[S_OPS], *plus = streams + s_at[S_PLUS], *ptext = streams + s_at[S_PTEXT];
	// the counts: marks and their scans, tlen and its scan, the literals
	uint64_t *sa = nullptr, *sb = nullptr, *st = nullptr, *sp = nullptr, *sl = nullptr, *seg_op = nullptr, *rec = nullptr;
	MCOM_HIP(ctx, B.get(&sa, 2 * (m + 1) * 8)); sb = sa + m + 1;
	MCOM_HIP(ctx, B.get(&st, (T + 1) * 8));
	MCOM_HIP(ctx, B.get(&sp, (n + 1) * 8));
	MCOM_LAUNCH(k_name_marks, dim3(blocks_for(m + 1)), dim3(NM_THREADS), 0, ctx->stream, ops, m, sa, sb, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_LAUNCH(k_name_bytes64, dim3(blocks_for(T + 1)), dim3(NM_THREADS), 0, ctx->stream, (const uint8_t*)(streams + s_at[S_TLEN]), T, st);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_LAUNCH(k_name_plus, dim3(blocks_for(n + 1)), dim3(NM_THREADS), 0, ctx->stream, plus, n, sp, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	if ((rc = mcom_scan64(ctx, sa, sa, m + 1, nullptr)) || (rc = mcom_scan64(ctx, sb, sb, m + 1, nullptr)) || (rc = mcom_scan64(ctx, st, st, T + 1, nullptr)) ||
	    (rc = mcom_scan64(ctx, sp, sp, n + 1, nullptr))) return rc;
	uint64_t ta = 0, tb = 0, tt = 0, n_lit = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&ta, sa + m, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tb, sb + m, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&tt, st + T, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&n_lit, sp + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return refuse("an op above 5, a last op that is not END or a '+' kind above 2", flag);
	if ((ta >> 32) != n || (ta & 0xFFFFFFFFu) != T || (tb >> 32) != raw[S_DELTA] || 4 * (tb & 0xFFFFFFFFu) != raw[S_NUM]) return refuse("the ops do not add up to the streams");
	if (tt != raw[S_TEXT]) return refuse("the text lengths do not add up to the text");
	if (n_lit > raw[S_PTEXT]) return refuse("more literals than ptext holds");
	MCOM_HIP(ctx, B.get(&sl, (n_lit + 1) * 8));
	MCOM_LAUNCH(k_name_bytes64, dim3(blocks_for(n_lit + 1)), dim3(NM_THREADS), 0, ctx->stream, ptext, n_lit, sl);
	MCOM_LAUNCH_CHECK(ctx);
	if ((rc = mcom_scan64(ctx, sl, sl, n_lit + 1, nullptr))) return rc;
	uint64_t lit_bytes = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&lit_bytes, sl + n_lit, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (n_lit + lit_bytes != raw[S_PTEXT]) return refuse("the literals do not use up ptext");
	if (raw[S_TEXT]) { MCOM_LAUNCH(k_name_newline, dim3(grid_capped(ctx, raw[S_TEXT])), dim3(NM_THREADS), 0, ctx->stream, (const uint8_t*)(streams + s_at[S_TEXT]), raw[S_TEXT], d_flag); MCOM_LAUNCH_CHECK(ctx); }
	if (lit_bytes) { MCOM_LAUNCH(k_name_newline, dim3(grid_capped(ctx, lit_bytes)), dim3(NM_THREADS), 0, ctx->stream, ptext + n_lit, lit_bytes, d_flag); MCOM_LAUNCH_CHECK(ctx); }
	// where every segment begins, then the two walks
	MCOM_HIP(ctx, B.get(&seg_op, (n_seg + 1) * 8));
	MCOM_HIP(ctx, hipMemsetAsync(seg_op, 0xFF, (n_seg + 1) * 8, ctx->stream));
	MCOM_LAUNCH(k_name_segstart, dim3(blocks_for(m)), dim3(NM_THREADS), 0, ctx->stream, ops, m, (const uint64_t*)sa, hd.rps, n_seg, seg_op);
	MCOM_LAUNCH_CHECK(ctx);
	if (d_rec_off) rec = d_rec_off; else MCOM_HIP(ctx, B.get(&rec, (n + 1) * 8));
	MCOM_HIP(ctx, hipMemsetAsync(rec, 0, (n + 1) * 8, ctx->stream));
	NmDecodeArgs A;
	A.v = View{ ops, streams + s_at[S_DELTA], streams + s_at[S_NUM], streams + s_at[S_TLEN], streams + s_at[S_TEXT], m, raw[S_DELTA], raw[S_NUM] / 4, T, raw[S_TEXT] };
	A.plus = plus; A.ptext = ptext; A.n_ptext = raw[S_PTEXT]; A.n_lit = n_lit;
	A.sa = sa; A.sb = sb; A.st = st; A.sp = sp; A.sl = sl; A.seg_op = seg_op;
	A.n = n; A.n_seg = n_seg; A.text_len = hd.text_len; A.rps = hd.rps;
	if (mstart) {
		MCOM_LAUNCH(k_name_walk_mate<0>, dim3(blocks_for(n)), dim3(NM_THREADS), 0, ctx->stream, A, d_mate, mate_len, (const uint64_t*)mstart, rec, (uint8_t*)nullptr, d_flag);
	} else {
		MCOM_LAUNCH(k_name_walk<0>, dim3(blocks_for(n_seg, NM_WALK_THREADS)), dim3(NM_WALK_THREADS), 0, ctx->stream, A, rec, (uint8_t*)nullptr, d_flag);
	}
	MCOM_LAUNCH_CHECK(ctx);
	if ((rc = mcom_scan64(ctx, rec, rec, n + 1, nullptr))) return rc;
	uint64_t total = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&total, rec + n, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return refuse("corrupt member", flag);
	if (total != hd.text_len) return refuse("the records do not add up to the text");
	if (mstart) {
		MCOM_LAUNCH(k_name_walk_mate<1>, dim3(blocks_for(n)), dim3(NM_THREADS), 0, ctx->stream, A, d_mate, mate_len, (const uint64_t*)mstart, rec, d_text, d_flag);
	} else {
		MCOM_LAUNCH(k_name_walk<1>, dim3(blocks_for(n_seg, NM_WALK_THREADS)), dim3(NM_WALK_THREADS), 0, ctx->stream, A, rec, d_text, d_flag);
	}
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) return refuse("corrupt member", flag);
	uint32_t crc = 0;
	if ((rc = mcom_device_crc32(ctx, d_text, hd.text_len, &crc))) return rc;
	if (crc != hd.crc) return refuse("CRC mismatch");
	return MCOM_OK;
}

extern "C" int mcom_name_decode(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, uint8_t *d_text, uint64_t cap, uint64_t *text_len, uint64_t *n_records, uint64_t *d_rec_off)
{
	return name_decode_impl(ctx, d_in, in_len, false, nullptr, 0, d_text, cap, text_len, n_records, d_rec_off);
}

extern "C" int mcom_name_decode_mate(mcom_ctx *ctx, const uint8_t *d_in, uint64_t in_len, const uint8_t *d_mate, uint64_t mate_len, uint8_t *d_text, uint64_t cap, uint64_t *text_len,
                                     uint64_t *n_records)
{
	return name_decode_impl(ctx, d_in, in_len, true, d_mate, mate_len, d_text, cap, text_len, n_records, nullptr);
}

extern "C" int mcom_name_text_offsets(mcom_ctx *ctx, const uint8_t *d_text, uint64_t text_len, uint64_t n, uint64_t *d_rec_off)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_rec_off || (text_len && !d_text)) return mcom_fail(ctx, MCOM_E_ARG, "name_text_offsets: null pointer");
	if (n > N_MAX || text_len < 2 * n || (n == 0 && text_len)) return mcom_fail(ctx, MCOM_E_ARG, "name_text_offsets: %llu bytes are not the two lines of each of %llu records", (unsigned long long)text_len, (unsigned long long)n);
	if (n == 0) { MCOM_HIP(ctx, hipMemsetAsync(d_rec_off, 0, 8, ctx->stream)); MCOM_HIP(ctx, mcom_stream_sync(ctx)); return MCOM_OK; }
	Blocks B(ctx);
	int rc;
	uint64_t lines = 0, *start = nullptr; uint32_t *d_flag = nullptr, flag[2] = {0, 0};
	if ((rc = mcom_decode_line_index(ctx, d_text, text_len, nullptr, 0, &lines, nullptr))) return rc;
	if (lines != 2 * n) return mcom_fail(ctx, MCOM_E_ARG, "name_text_offsets: %llu lines, not the two lines of each of %llu records", (unsigned long long)lines, (unsigned long long)n);
	MCOM_HIP(ctx, B.get(&start, (2 * n + 1) * 8));
	MCOM_HIP(ctx, B.get(&d_flag, 8));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
	if ((rc = mcom_decode_line_index(ctx, d_text, text_len, start, 2 * n, &lines, d_flag + 1))) return rc;
	MCOM_LAUNCH(k_name_lines, dim3(blocks_for(n + 1)), dim3(NM_THREADS), 0, ctx->stream, (const uint64_t*)start, n, text_len, d_rec_off, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(flag, d_flag, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag[0] || flag[1]) return mcom_fail(ctx, MCOM_E_ARG, "name_text_offsets: the text is not two complete lines of at most 255 bytes per record (flag 0x%x)", flag[0]);
	return MCOM_OK;
}

// ---- FASTQ text <-> name text (the two ends of `minicom -N`) ----------------------------------------------------------------------------
//   k_fastq_name_lens   one lane per record: lines 4r and 4r + 2 of a line index checked ('@', '+', at most 255 bytes behind them),
//                       len[r] = the bytes the record takes in the name text (0 for a flagged record)
//   k_fastq_name_copy   sixteen lanes per record: the two lines without their first byte, each with its newline, at the record's offset
//   k_fastq_emit_named  sixteen lanes per record: `@<name>\n<read>\n+<text>\n<qualities>\n` at (2 L + 4) r + the record's offset in the
//                       name text; the name ends at the first newline of the record's piece of name text
//   k_name_compare      sixteen lanes per record: two name texts with their record offsets, the differing records counted, the lowest kept
__global__ __launch_bounds__(NM_THREADS) void k_fastq_name_lens(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint64_t *__restrict__ start, uint64_t first_record, uint64_t n_records,
                                                                uint64_t *__restrict__ len, uint32_t *__restrict__ flag)
{
	const uint64_t r = (uint64_t)blockIdx.x * NM_THREADS + threadIdx.x;
	if (r > n_records) return;
	uint64_t v = 0;
	if (r < n_records) {
		const uint64_t a = start[4 * r], b = start[4 * r + 1], c = start[4 * r + 2], d = start[4 * r + 3], e = start[4 * r + 4];
		uint32_t bad = 0;
		if (!(a < b && b < c && c < d && d < e && e <= n_bytes)) bad = MCOM_FASTQ_F_LENGTH;     // (cannot be: the index is made of this text)
		else {
			if (b - 1 - a < 1 || text[a] != '@') bad |= MCOM_FASTQ_F_NAME;
			if (d - 1 - c < 1 || text[c] != '+') bad |= MCOM_FASTQ_F_PLUS;
			if (!bad && (b - 2 - a > NM_NAME_MAX || d - 2 - c > NM_NAME_MAX)) bad |= MCOM_FASTQ_F_LONG;
		}
		if (bad) { atomicOr(&flag[0], bad); atomicMin(&flag[1], (uint32_t)(first_record + r)); }
		else v = (b - 1 - a) + (d - 1 - c);                                    // each line without its first byte, with its newline
	}
	len[r] = v;
}
__global__ __launch_bounds__(NM_THREADS) void k_fastq_name_copy(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start, uint64_t n_records, const uint64_t *__restrict__ off,
                                                                uint8_t *__restrict__ names, uint64_t cap)
{
	const uint64_t r = ((uint64_t)blockIdx.x * NM_THREADS + threadIdx.x) / NM_G;
	const uint32_t lane = threadIdx.x % NM_G;
	if (r >= n_records) return;
	const uint64_t at = off[r], end = off[r + 1];
	if (end <= at || end > cap) return;                                        // a flagged record takes no room
	const uint64_t a = start[4 * r], b = start[4 * r + 1], c = start[4 * r + 2], d = start[4 * r + 3];
	const uint64_t nl = b - 1 - a, pl = d - 1 - c;                              // with their newlines
	if (nl + pl != end - at) return;
	for (uint64_t j = lane; j < nl; j += NM_G) names[at + j] = text[a + 1 + j];
	for (uint64_t j = lane; j < pl; j += NM_G) names[at + nl + j] = text[c + 1 + j];
}

extern "C" int mcom_fastq_name_text(mcom_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_line_start, uint64_t first_record, uint64_t n_records,
                                    uint8_t *d_names, uint64_t cap, uint64_t *bytes, uint64_t *d_rec_off, uint32_t *d_flag)
{
	if (!ctx) return MCOM_E_ARG;
	if (!d_flag || !bytes || !d_rec_off || (n_records && (!d_text || !d_line_start))) return mcom_fail(ctx, MCOM_E_ARG, "fastq_name_text: null pointer");
	*bytes = 0;
	if (first_record + n_records >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_name_text: %llu records from %llu", (unsigned long long)n_records, (unsigned long long)first_record);
	MCOM_LAUNCH(k_fastq_name_lens, dim3(blocks_for(n_records + 1)), dim3(NM_THREADS), 0, ctx->stream, d_text, n_bytes, d_line_start, first_record, n_records, d_rec_off, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	int rc = mcom_scan64(ctx, d_rec_off, d_rec_off, n_records + 1, nullptr);
	if (rc) return rc;
	uint64_t total = 0;
	MCOM_HIP(ctx, hipMemcpyAsync(&total, d_rec_off + n_records, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*bytes = total;
	if (!d_names || !total) return MCOM_OK;
	if (total > cap) return mcom_fail(ctx, MCOM_E_OVERFLOW, "fastq_name_text: %llu bytes of name text, room for %llu", (unsigned long long)total, (unsigned long long)cap);
	MCOM_LAUNCH(k_fastq_name_copy, dim3(blocks_for(n_records * NM_G)), dim3(NM_THREADS), 0, ctx->stream, d_text, d_line_start, n_records, (const uint64_t*)d_rec_off, d_names, cap);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	return MCOM_OK;
}

// the first newline of a record's piece of name text [at, end), found by the sixteen lanes of the record together (end when there is none)
__device__ __forceinline__ uint64_t nm_name_end(const uint8_t *names, uint64_t at, uint64_t end, uint32_t lane)
{
	uint32_t best = 0xFFFFFFFFu;
	for (uint64_t j = at + lane; j < end && best == 0xFFFFFFFFu; j += NM_G) if (names[j] == '\n') best = (uint32_t)(j - at);
#pragma unroll
	for (int o = NM_G / 2; o; o >>= 1) { const uint32_t other = __shfl_xor(best, o, NM_G); best = other < best ? other : best; }
	return best == 0xFFFFFFFFu ? end : at + best;
}

__global__ __launch_bounds__(NM_THREADS) void k_fastq_emit_named(const uint8_t *__restrict__ reads, uint64_t read_pitch, const uint8_t *__restrict__ quals, uint64_t qual_pitch,
                                                                 const uint8_t *__restrict__ names, uint64_t names_bytes, const uint64_t *__restrict__ off, uint64_t count, uint32_t L,
                                                                 uint8_t *__restrict__ out, uint64_t out_bytes, uint32_t *__restrict__ flag)
{
	const uint64_t r = ((uint64_t)blockIdx.x * NM_THREADS + threadIdx.x) / NM_G;
	const uint32_t lane = threadIdx.x % NM_G;
	if (r >= count) return;
	const uint64_t base = off[0], at = off[r], end = off[r + 1];
	const uint64_t o0 = r * (2 * (uint64_t)L + 4) + (at - base);
	// (all sixteen lanes of a record see the same offsets and take the same way)
	if (at < base || end < at + 2 || end - at > 2 * (uint64_t)NM_NAME_MAX + 2 || end > names_bytes || o0 + 2 * (uint64_t)L + 4 + (end - at) > out_bytes) { if (lane == 0) atomicOr(flag, 1u); return; }
	const uint64_t mid = nm_name_end(names, at, end - 1, lane);                // the name's newline; the text's is the piece's last byte
	const uint32_t nl = (uint32_t)(mid - at), pl = (uint32_t)(end - 1 - at) - nl - (mid < end - 1 ? 1u : 0u);
	if (mid >= end - 1 || names[end - 1] != '\n') { if (lane == 0) atomicOr(flag, 1u); return; }
	uint8_t *o = out + o0;
	const uint8_t *rd = reads + r * read_pitch, *ql = quals + r * qual_pitch;
	uint8_t *o_read = o + 1 + nl + 1, *o_plus = o_read + L + 1, *o_qual = o_plus + 1 + pl + 1;
	for (uint32_t j = lane; j < nl; j += NM_G) o[1 + j] = names[at + j];
	for (uint32_t j = lane; j < pl; j += NM_G) o_plus[1 + j] = names[mid + 1 + j];
	for (uint32_t j = lane; j < L; j += NM_G) { o_read[j] = rd[j]; o_qual[j] = ql[j]; }
	if (lane == 0) { o[0] = '@'; o[1 + nl] = '\n'; o_read[L] = '\n'; o_plus[0] = '+'; o_plus[1 + pl] = '\n'; o_qual[L] = '\n'; }
}

extern "C" int mcom_fastq_emit_named(mcom_ctx *ctx, const uint8_t *d_reads, uint64_t read_pitch, const uint8_t *d_quals, uint64_t qual_pitch, const uint8_t *d_names, uint64_t names_bytes,
                                     const uint64_t *d_rec_off, uint64_t count, uint32_t L, uint8_t *d_out, uint64_t *bytes)
{
	if (!ctx) return MCOM_E_ARG;
	if (!bytes || (count && !d_rec_off)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_named: null pointer");
	*bytes = 0;
	if (L < 1 || L > 256 || read_pitch < L || qual_pitch < L || count >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_named: L %u, %llu records", L, (unsigned long long)count);
	if (!count) return MCOM_OK;
	uint64_t ends[2] = {0, 0};
	MCOM_HIP(ctx, hipMemcpyAsync(&ends[0], d_rec_off, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, hipMemcpyAsync(&ends[1], d_rec_off + count, 8, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (ends[1] < ends[0] + 2 * count || ends[1] > names_bytes) return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_named: the record offsets %llu .. %llu do not lie in %llu bytes of name text",
	                                                                           (unsigned long long)ends[0], (unsigned long long)ends[1], (unsigned long long)names_bytes);
	const uint64_t total = count * (2 * (uint64_t)L + 4) + (ends[1] - ends[0]);
	*bytes = total;
	if (!d_out) return MCOM_OK;
	if (!d_reads || !d_quals || !d_names) { *bytes = 0; return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_named: null pointer"); }
	Blocks B(ctx);
	uint32_t *d_flag = nullptr, flag = 0;
	MCOM_HIP(ctx, B.get(&d_flag, 4));
	MCOM_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
	MCOM_LAUNCH(k_fastq_emit_named, dim3(blocks_for(count * NM_G)), dim3(NM_THREADS), 0, ctx->stream, d_reads, read_pitch, d_quals, qual_pitch, d_names, names_bytes, d_rec_off, count, L, d_out, total, d_flag);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	if (flag) { *bytes = 0; return mcom_fail(ctx, MCOM_E_ARG, "fastq_emit_named: the record offsets do not describe two lines of at most 255 bytes per record"); }
	return MCOM_OK;
}

// res[0] = differing records, res[1] = the lowest of them
__global__ __launch_bounds__(NM_THREADS) void k_name_compare(const uint8_t *__restrict__ a, const uint64_t *__restrict__ off_a, uint64_t bytes_a, const uint8_t *__restrict__ b, const uint64_t *__restrict__ off_b,
                                                             uint64_t bytes_b, uint64_t n, unsigned long long *__restrict__ res)
{
	const uint64_t r = ((uint64_t)blockIdx.x * NM_THREADS + threadIdx.x) / NM_G;
	const uint32_t lane = threadIdx.x % NM_G;
	if (r >= n) return;
	const uint64_t a0 = off_a[r], a1 = off_a[r + 1], b0 = off_b[r], b1 = off_b[r + 1];
	uint32_t diff = 0;
	if (a1 < a0 || b1 < b0 || a1 > bytes_a || b1 > bytes_b || a1 - a0 != b1 - b0) diff = 1;
	else for (uint64_t j = lane; j < a1 - a0 && j < 2 * (uint64_t)NM_NAME_MAX + 2; j += NM_G) diff |= a[a0 + j] != b[b0 + j];
	if (!diff && a1 - a0 > 2 * (uint64_t)NM_NAME_MAX + 2) diff = 1;             // (no record of a name text is longer)
#pragma unroll
	for (int o = NM_G / 2; o; o >>= 1) diff |= __shfl_xor(diff, o, NM_G);
	if (diff && lane == 0) { atomicAdd(&res[0], 1ull); atomicMin(&res[1], (unsigned long long)r); }
}

extern "C" int mcom_name_compare(mcom_ctx *ctx, const uint8_t *d_a, const uint64_t *d_off_a, uint64_t bytes_a, const uint8_t *d_b, const uint64_t *d_off_b, uint64_t bytes_b, uint64_t n,
                                 uint64_t *differing, uint64_t *first_diff)
{
	if (!ctx) return MCOM_E_ARG;
	if (!differing || !first_diff || (n && (!d_off_a || !d_off_b))) return mcom_fail(ctx, MCOM_E_ARG, "name_compare: null pointer");
	*differing = 0; *first_diff = ~(uint64_t)0;
	if (!n) return MCOM_OK;
	if (n >= ((uint64_t)1 << 32)) return mcom_fail(ctx, MCOM_E_ARG, "name_compare: %llu records", (unsigned long long)n);
	Blocks B(ctx);
	unsigned long long *d_res = nullptr, res[2] = {0, ~0ull};
	MCOM_HIP(ctx, B.get(&d_res, 16));
	MCOM_HIP(ctx, hipMemcpyAsync(d_res, res, 16, hipMemcpyHostToDevice, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	MCOM_LAUNCH(k_name_compare, dim3(blocks_for(n * NM_G)), dim3(NM_THREADS), 0, ctx->stream, d_a, d_off_a, bytes_a, d_b, d_off_b, bytes_b, n, d_res);
	MCOM_LAUNCH_CHECK(ctx);
	MCOM_HIP(ctx, hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, ctx->stream));
	MCOM_HIP(ctx, mcom_stream_sync(ctx));
	*differing = res[0]; *first_diff = res[1];
	return MCOM_OK;
}
