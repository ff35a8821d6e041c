// minicom_amd/host/mcom_decompress_gpu.cpp -- the three decoders of mcom_decompress.cpp with the reads rebuilt on the device.
//
// Same stream files in, byte-identical output files out; mcom_decompress.cpp stays the specification (what it accepts is accepted,
// what it refuses is refused) and the cross-check.  The work is cut in two:
//   A. every stream file is read and uploaded whole; line indices, member tables and destination rows are made by the scans of
//      csrc/decode.hip; the counts they give (lines against members, id words, file bits, n_seq, half, bases of ref.bin) and the flag
//      word the kernels raise are compared on the host.  An archive that fails here is refused before anything is decoded.
//   B. one mcom_decode_reads per list / stream set writes its reads into a table of rows in HBM (L characters and a newline each:
//      the file image); the table comes back through two page-locked buffers, the copy of piece i + 1 under the write of piece i.
//   B'. a record range (`minicom -d -R`): A unchanged, then mcom_range_check_dest over every source -- the placement
//      check of the full decode -- and mcom_range_decode_reads into a table of the window's rows alone: count x (L + 1) bytes, not n x (L + 1).
//   C. what becomes of the rows is the caller's tail: the three decoders write the file(s) (write_files); mcomh_verify_gpu compares the table,
//      still in HBM, with the reads of the FASTQ file(s) (compare_rows over csrc/verify.hip) and writes nothing.
// The only serial step is the chain of contig headers in beg_pos.bin (mcom_decode_walk_headers: four bytes read per contig).
// No output file is left behind by a refused archive; there is no fall back to the host decoder.
#include "../../include/mcom_host.h"
#include "../../include/mcom.h"
#include "mcom_fastq.hpp"
#include "mcom_ragged.hpp"
#include "mcom_agree.hpp"
#include "mcom_range.hpp"
#include "mcom_streams.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

using namespace mcom_streams;                         // Mode, what a folder of each mode holds and its loaders: shared with the host decoder

namespace {

size_t PIECE_BYTES = (size_t)64 << 20;                // one page-locked buffer; two of them bound the host memory of the download
                                                        // (mcomh_test_decoder_piece_bytes, include/mcom_test.h, lets a test cross pieces with a few thousand records)

double g_times[8];                                      // ms: read files | upload + indices + destinations | decode, wall | decode, device events |
                                                        //     download + write, wall | of that inside fwrite | whole call | unused
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Refuse { const char *why; };                     // thrown inside run(), caught there: never crosses the C boundary

// device memory and page-locked buffers of one call, released when it ends however it ends
struct Arena {
	std::vector<void*> dev, pinned;
	hipEvent_t ev[2] = {nullptr, nullptr};
	mcom_ctx *ctx = nullptr;
	struct SetRef { const uint8_t *d_ref; uint64_t ref_bytes, bases; };
	std::vector<SetRef> set_refs;                           // the ref.bin of every stream set in HBM and the bases its contigs hold (run(), A.2)
	~Arena()
	{
		if (ctx) (void)mcom_sync(ctx);
		for (void *p : dev) (void)hipFree(p);
		for (void *p : pinned) (void)hipHostFree(p);
		for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
		if (ctx) mcom_destroy(ctx);
	}
	template <class T> T *alloc(size_t n)
	{
		void *p = nullptr;
		if (hipMalloc(&p, (n ? n : 1) * sizeof(T) + 16) != hipSuccess) throw Refuse{"the card has no room for the stream files and the rows"};
		dev.push_back(p);
		return (T*)p;
	}
	template <class T> T *upload(const T *h, size_t n)
	{
		T *d = alloc<T>(n);
		if (n && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw Refuse{"upload failed"};
		return d;
	}
};

// one run of reads that a single mcom_decode_reads call rebuilds
struct Seg {
	mcom_decode_src src;
	uint64_t n = 0;
	const uint64_t *d_dest = nullptr; uint64_t dest0 = 0;
	uint64_t ref_bases = 0;                                                 // a stream set: the bases of its contigs (mcom_decode_member_table)
};

// An output path that ends in `.gz` is written as BGZF: the pieces of text never leave the card, their members do.
// The whole blocks of (carry + piece) go through mcom_bgzf_encode, what is left below one block is carried in front of the next piece and
// the last piece is closed with the empty member -- so block k of the file holds its bytes [65280 k, ...) whatever the piece size, and
// the file equals mcomh_bgzf_encode of the plain output byte for byte.
bool gz_path(const char *path) { const size_t n = path ? strlen(path) : 0; return n >= 3 && !strcmp(path + n - 3, ".gz"); }
struct GzSink {
	enum { BLOCK = 65280 };
	Arena &A;
	uint8_t *d_text = nullptr, *d_members = nullptr, *pin = nullptr;
	size_t room = 0, cap = 0, carry = 0;
	explicit GzSink(Arena &a) : A(a)
	{
		room = PIECE_BYTES + BLOCK; cap = (size_t)mcom_bgzf_bound(room);
		d_text = A.alloc<uint8_t>(room); d_members = A.alloc<uint8_t>(cap);
		void *p = nullptr;
		if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) throw Refuse{"no page-locked memory"};
		A.pinned.push_back(p); pin = (uint8_t*)p;
	}
	// `bytes` (at most a piece) of text on the device, the file's last ones when `last`; false when a call or the write failed
	bool feed(const uint8_t *d_piece, size_t bytes, bool last, FILE *out)
	{
		if (bytes > PIECE_BYTES || carry >= BLOCK) return false;
		if (bytes && hipMemcpy(d_text + carry, d_piece, bytes, hipMemcpyDeviceToDevice) != hipSuccess) return false;
		if (hipDeviceSynchronize() != hipSuccess) return false;
		const size_t have = carry + bytes, whole = last ? have : have - have % BLOCK;
		uint64_t len = 0;
		if (whole || last) {
			if (mcom_bgzf_encode(A.ctx, d_text, whole, d_members, cap, &len, last ? MCOM_BGZF_EOF : 0)) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); return false; }
			if (hipMemcpy(pin, d_members, (size_t)len, hipMemcpyDeviceToHost) != hipSuccess) return false;
		}
		carry = have - whole;
		if (carry && whole && (hipMemcpy(d_text, d_text + whole, carry, hipMemcpyDeviceToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) return false;   // (carry < BLOCK <= whole: the two do not overlap)
		const double tw = now_ms();
		const bool wrote = fwrite(pin, 1, (size_t)len, out) == len;
		g_times[5] += now_ms() - tw;
		return wrote;
	}
};

void ok(mcom_ctx *ctx, int rc) { if (rc) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(ctx)); throw Refuse{"a device call failed"}; } }

struct Text { const uint8_t *d = nullptr; uint64_t bytes = 0, lines = 0; const uint64_t *start = nullptr; };

Text index_text(Arena &A, const std::vector<uint8_t> &h, uint32_t *d_flag)
{
	Text t;
	t.bytes = h.size();
	t.d = A.upload(h.data(), h.size());
	ok(A.ctx, mcom_decode_line_index(A.ctx, t.d, t.bytes, nullptr, 0, &t.lines, d_flag));
	uint64_t *st = A.alloc<uint64_t>(t.lines + 1);
	uint64_t again = 0;
	ok(A.ctx, mcom_decode_line_index(A.ctx, t.d, t.bytes, st, t.lines, &again, d_flag));
	t.start = st;
	return t;
}

uint32_t read_flag(Arena &A, const uint32_t *d_flag)
{
	uint32_t f = 0;
	ok(A.ctx, mcom_sync(A.ctx));
	if (hipMemcpy(&f, d_flag, 4, hipMemcpyDeviceToHost) != hipSuccess) throw Refuse{"cannot read the flag word"};
	return f;
}

// Phases A and B for the three decoders and for the verifier alike; `tail` gets the rows while they are still in HBM: 0 = done, else the call fails
using Tail = std::function<int(Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L)>;
// between B and C, for the callers that need what the rows were decoded from (the agreement mask): the segments of
// an archive that has passed every check of A and B.  It throws Refuse like everything inside run().
using Between = std::function<void(Arena &A, const std::vector<Seg> &segs, uint64_t n_rows, int L, uint32_t *d_flag)>;

// a record range: run() decodes the rows [first, first + count) alone -- pair: and [half + first, half + first + count), the same records of
// the second file of a pair kept in input order, behind them -- and hands the tail that table.  It clips count at the last record and
// states n_records, the records (of one file) in the archive, for the tails that set the side members against it.
struct Window { uint64_t first, count; bool pair; uint64_t n_records = 0; };
// folder/pe_order.txt of a pair kept in input order: the pairs it states, which must be half of n_rows
uint64_t pairs_of(const char *folder, uint64_t n_rows)
{
	uint64_t n_pairs = 0;
	if (!pair_count(folder, n_rows, n_pairs)) throw Refuse{"no pe_order.txt that states half the reads' number: not a pair kept in input order"};
	return n_pairs;
}

int run(Mode mode, const char *folder, int device, const Tail &tail, const Between *between = nullptr, Window *win = nullptr)
{
	const double t_begin = now_ms();
	memset(g_times, 0, sizeof(g_times));
	const std::string dir(folder);
	// ---- info.txt and the first size checks, by the host routes' own code (mcom_streams.hpp)
	StreamInfo I;
	if (!read_info(mode, dir, I) || !counts_fit(mode, dir, I)) return -1;
	const int L = I.L, nth = I.nth;
	const long na = I.na, nt = I.nt, nn = I.nn, half = I.half;
	const unsigned long n_seq = I.n_seq;

	// ---- the stream files, whole
	double t0 = now_ms();
	SectionFiles lists[N_SECTIONS];
	SetFiles sp;                                                            // paired end: the sections' file bits and mate numbers
	std::vector<SetFiles> sets((size_t)nth);
	for (int s = 0; s < N_SECTIONS; ++s) if (!load_section(mode, dir, s, lists[s])) return -1;
	if (mode == PE && !load_pairing(dir, ".sp", sp)) return -1;
	for (int th = 0; th < nth; ++th) if (!load_set(mode, dir, th, sets[(size_t)th])) return -1;
	g_times[0] = now_ms() - t0;
	// (the order of SECTIONS: three counted, three near-constant, the N reads, the unclustered reads)
	const SectionFiles *h_counted = lists, *h_near = lists + 3;
	const std::vector<uint8_t> &h_nseq = lists[6].data, &h_nids = lists[6].ids, &h_single = lists[7].data, &h_sids = lists[7].ids, &h_fsp = sp.fb, &h_psp = sp.pe;
	// the serial part: the chain of contig headers
	std::vector<std::vector<uint64_t>> moff((size_t)nth);
	std::vector<uint64_t> n_contigs((size_t)nth), n_members((size_t)nth);
	for (int th = 0; th < nth; ++th) {
		const SetFiles &s = sets[(size_t)th];
		if (mcom_decode_walk_headers(s.pos.data(), s.pos.size(), nullptr, 0, &n_contigs[th], &n_members[th])) return -1;
		moff[th].resize(n_contigs[th] + 1);
		if (mcom_decode_walk_headers(s.pos.data(), s.pos.size(), moff[th].data(), n_contigs[th], &n_contigs[th], &n_members[th])) return -1;
	}

	// ---- the card
	Arena A;
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
			fprintf(stderr, "minicom gpu decoder: no GPU %d (%d visible); the host decoder is a call of its own\n", device, n_dev);
			return -1;
		}
		if (mcom_create(&A.ctx, device, nullptr)) { fprintf(stderr, "minicom gpu decoder: cannot create a context on GPU %d\n", device); A.ctx = nullptr; return -1; }
	}
	try {
		t0 = now_ms();
		uint32_t *d_flag = A.alloc<uint32_t>(1);
		if (hipMemset(d_flag, 0, 4) != hipSuccess) throw Refuse{"memset failed"};
		std::vector<Seg> segs;
		auto blank = [&]() { Seg s; memset(&s.src, 0, sizeof(s.src)); return s; };
		const char bases[3] = {'A', 'T', 'N'};
		const long counted[3] = {na, nt, nn};
		// A.1 the lists: counted reads, near-constant reads, N reads, unclustered reads
		for (int q = 0; q < 3; ++q) {
			Seg s = blank(); s.src.ref_const = bases[q]; s.n = (uint64_t)counted[q];
			if (mode == ORDER) {
				if (h_counted[q].ids.size() / 4 < s.n) throw Refuse{"fewer ids than counted reads"};
				const uint32_t *d = A.upload((const uint32_t*)h_counted[q].ids.data(), (size_t)s.n);
				uint64_t *dest = A.alloc<uint64_t>(s.n);
				ok(A.ctx, mcom_decode_list_ids(A.ctx, d, s.n, dest));
				s.d_dest = dest;
			}
			segs.push_back(s);
		}
		auto text_seg = [&](const std::vector<uint8_t> &h, int ref_const, int verbatim, const std::vector<uint8_t> &h_ids) {
			const Text t = index_text(A, h, d_flag);
			Seg s = blank();
			s.src.d_text = t.d; s.src.text_bytes = t.bytes; s.src.d_line_start = t.start; s.src.verbatim = verbatim; s.src.ref_const = ref_const;
			s.n = t.lines;
			ok(A.ctx, mcom_decode_check_lines(A.ctx, t.d, t.bytes, t.start, s.n, L, verbatim, d_flag));
			if (mode == ORDER) {
				if (h_ids.size() / 4 < s.n) throw Refuse{"fewer ids than lines"};
				const uint32_t *d = A.upload((const uint32_t*)h_ids.data(), (size_t)s.n);
				uint64_t *dest = A.alloc<uint64_t>(s.n);
				ok(A.ctx, mcom_decode_list_ids(A.ctx, d, s.n, dest));
				s.d_dest = dest;
			}
			segs.push_back(s);
		};
		for (int q = 0; q < 3; ++q) text_seg(h_near[q].data, bases[q], 0, h_near[q].ids);
		auto single_seg = [&]() {
			Seg s = blank();
			s.n = (uint64_t)h_single.size() * 4 / (uint64_t)L;                 // whole reads only: the last byte may be padded
			if (mode == ORDER && h_sids.size() / 4 < s.n) s.n = h_sids.size() / 4;  // (the host route stops, without an error, where the ids end)
			s.src.d_ref = A.upload(h_single.data(), h_single.size()); s.src.ref_bytes = h_single.size();
			if (mode == ORDER) {
				const uint32_t *d = A.upload((const uint32_t*)h_sids.data(), (size_t)s.n);
				uint64_t *dest = A.alloc<uint64_t>(s.n);
				ok(A.ctx, mcom_decode_list_ids(A.ctx, d, s.n, dest));
				s.d_dest = dest;
			}
			segs.push_back(s);
		};
		// the host routes take the N reads before the unclustered ones, except -p (ids of their own: the order does not show)
		if (mode == ORDER) { single_seg(); text_seg(h_nseq, 'N', 1, h_nids); }
		else { text_seg(h_nseq, 'N', 1, h_nids); single_seg(); }
		const size_t n_list_segs = segs.size();
		// A.2 the stream sets
		for (int th = 0; th < nth; ++th) {
			const SetFiles &f = sets[(size_t)th];
			const uint64_t nm = n_members[th], nc = n_contigs[th];
			Seg s = blank();
			s.n = nm;
			const Text t = index_text(A, f.dif, d_flag);
			if (t.lines < nm) throw Refuse{"fewer dif_char lines than members"};
			if (mode == ORDER && f.ids.size() / 4 < nm) throw Refuse{"fewer id words than members"};
			const uint8_t *d_bpos = A.upload(f.pos.data(), f.pos.size());
			const uint64_t *d_moff = A.upload(moff[th].data(), moff[th].size());
			uint32_t *cid = A.alloc<uint32_t>(nm), *pos = A.alloc<uint32_t>(nm);
			uint64_t *coff = A.alloc<uint64_t>(nc + 1);
			uint64_t ref_bases = 0;
			ok(A.ctx, mcom_decode_member_table(A.ctx, d_bpos, f.pos.size(), d_moff, nc, nm, L, cid, pos, coff, &ref_bases, d_flag));
			if (ref_bases > 4 * (uint64_t)f.ref.size()) throw Refuse{"ref.bin is shorter than its contigs"};
			s.ref_bases = ref_bases;
			ok(A.ctx, mcom_decode_check_lines(A.ctx, t.d, t.bytes, t.start, nm, L, 0, d_flag));
			s.src.d_text = t.d; s.src.text_bytes = t.bytes; s.src.d_line_start = t.start;
			s.src.d_ref = A.upload(f.ref.data(), f.ref.size()); s.src.ref_bytes = f.ref.size();
			A.set_refs.push_back({s.src.d_ref, s.src.ref_bytes, ref_bases});
			s.src.d_cid = cid; s.src.d_pos = pos; s.src.d_coff = coff; s.src.n_contigs = nc;
			s.src.d_dir = A.upload(f.dir.data(), f.dir.size()); s.src.dir_bytes = f.dir.size();
			if (mode == ORDER) {
				const uint32_t *d = A.upload((const uint32_t*)f.ids.data(), (size_t)nm);
				uint64_t *dest = A.alloc<uint64_t>(nm);
				ok(A.ctx, mcom_decode_member_ids(A.ctx, d, nm, d_moff, cid, pos, dest));
				s.d_dest = dest;
			}
			segs.push_back(s);
		}
		// A.3 rows
		uint64_t total = 0;
		for (const Seg &s : segs) total += s.n;
		uint64_t n_rows = total;
		if (mode == ORDER) { if (total != (uint64_t)n_seq) throw Refuse{"the streams do not hold n_seq reads"}; }
		if (mode == PE) {
			if (total != 2 * (uint64_t)half) throw Refuse{"the streams do not hold 2 x half reads"};
			// the eight lists share file.bin.sp / peids.bin.sp; every set has its own pair
			uint64_t zeros = 0, n_sp = 0;
			for (size_t i = 0; i < n_list_segs; ++i) n_sp += segs[i].n;
			{
				const uint8_t *fb = A.upload(h_fsp.data(), h_fsp.size());
				const uint32_t *pe = A.upload((const uint32_t*)h_psp.data(), h_psp.size() / 4);
				uint64_t *dest = A.alloc<uint64_t>(n_sp), ones = 0;
				ok(A.ctx, mcom_decode_pe_dest(A.ctx, fb, h_fsp.size(), 0, n_sp, pe, h_psp.size() / 4, 0, (uint64_t)half, dest, &ones, d_flag));
				uint64_t at = 0;
				for (size_t i = 0; i < n_list_segs; ++i) { segs[i].d_dest = dest + at; at += segs[i].n; }
				zeros = n_sp - ones;
			}
			for (int th = 0; th < nth; ++th) {
				const SetFiles &f = sets[(size_t)th];
				Seg &s = segs[n_list_segs + (size_t)th];
				const uint8_t *fb = A.upload(f.fb.data(), f.fb.size());
				const uint32_t *pe = A.upload((const uint32_t*)f.pe.data(), f.pe.size() / 4);
				uint64_t *dest = A.alloc<uint64_t>(s.n), ones = 0;
				ok(A.ctx, mcom_decode_pe_dest(A.ctx, fb, f.fb.size(), 0, s.n, pe, f.pe.size() / 4, zeros, (uint64_t)half, dest, &ones, d_flag));
				s.d_dest = dest;
				zeros += s.n - ones;
			}
			if (zeros != (uint64_t)half) throw Refuse{"the first file does not get half of the reads"};
		}
		if (mode == DEFAULT) { uint64_t at = 0; for (Seg &s : segs) { s.dest0 = at; at += s.n; } }
		// everything the files say about sizes has been checked: a raised flag refuses the archive before a read is decoded
		if (read_flag(A, d_flag)) throw Refuse{"the stream files are inconsistent"};
		// a range: the window's rows alone are made, so they alone must fit (the stream files and the tables above stay whole)
		uint64_t table_rows = n_rows;
		if (win) {
			if (mode != ORDER) throw Refuse{"a range needs the input order of a -p archive"};
			win->n_records = win->pair ? pairs_of(folder, n_rows) : n_rows;
			if (win->first > win->n_records) {
				fprintf(stderr, "minicom gpu decoder: the range begins at record %llu (from 0), the archive holds %llu\n", (unsigned long long)win->first, (unsigned long long)win->n_records);
				throw Refuse{"the range begins behind the last record"};
			}
			if (win->count > win->n_records - win->first) win->count = win->n_records - win->first;
			table_rows = (win->pair ? 2 : 1) * win->count;
		}
		const uint64_t row = (uint64_t)L + 1, table_bytes = table_rows * row;
		{
			size_t fr = 0, tot = 0;
			if (hipMemGetInfo(&fr, &tot) != hipSuccess || table_bytes + n_rows / 8 + ((size_t)64 << 20) > fr) {
				fprintf(stderr, "minicom gpu decoder: %llu rows of %d + 1 bytes do not fit the card (%zu bytes free)\n", (unsigned long long)table_rows, L, fr);
				throw Refuse{"the rows do not fit the card"};
			}
		}
		uint8_t *table = A.alloc<uint8_t>(table_bytes);
		uint32_t *seen = nullptr;
		if (mode != DEFAULT) {
			seen = A.alloc<uint32_t>(n_rows / 32 + 1);
			if (hipMemset(seen, 0, (n_rows / 32 + 1) * 4) != hipSuccess) throw Refuse{"memset failed"};
		}
		g_times[1] = now_ms() - t0;                                            // upload, indices and destinations (interleaved per stream)

		// ---- B. decode
		if (hipEventCreate(&A.ev[0]) != hipSuccess || hipEventCreate(&A.ev[1]) != hipSuccess) throw Refuse{"no events"};
		t0 = now_ms();
		(void)hipEventRecord(A.ev[0], nullptr);
		if (win) {
			// as many reads as rows (A.3): no destination outside and none twice means every row, of any window, exactly once
			for (const Seg &s : segs) ok(A.ctx, mcom_range_check_dest(A.ctx, s.d_dest, s.dest0, s.n, n_rows, seen, d_flag));
			for (int w = 0; w < (win->pair ? 2 : 1); ++w)
				for (const Seg &s : segs) ok(A.ctx, mcom_range_decode_reads(A.ctx, &s.src, s.n, L, s.d_dest, s.dest0, (uint64_t)w * win->n_records + win->first, win->count, table + (uint64_t)w * win->count * row, d_flag));
		} else {
			for (const Seg &s : segs) ok(A.ctx, mcom_decode_reads(A.ctx, &s.src, s.n, L, s.d_dest, s.dest0, table, n_rows, seen, d_flag));
		}
		(void)hipEventRecord(A.ev[1], nullptr);
		const uint32_t fl = read_flag(A, d_flag);
		{ float ms = 0; if (hipEventElapsedTime(&ms, A.ev[0], A.ev[1]) == hipSuccess) g_times[3] = ms; }
		g_times[2] = now_ms() - t0;
		if (fl) throw Refuse{"a read cannot be decoded or placed"};
		if (between) (*between)(A, segs, n_rows, L, d_flag);

		// ---- C. what becomes of the rows: the file(s), or the comparison of mcomh_verify_gpu
		if (tail(A, table, table_rows, win ? win->count : (uint64_t)half, L)) return -1;
	} catch (const Refuse &r) {
		fprintf(stderr, "minicom gpu decoder: %s refused: %s\n", folder, r.why);
		return -1;
	}
	g_times[6] = now_ms() - t_begin;
	return 0;
}

// ---- the agreement mask (`minicom -a Q[:C]`) of an archive run() has accepted: n_rows rows of (L + 7) / 8 bytes in
// HBM.  Per stream set one mcom_agree_coverage (its array lives until the set's mask rows are written) and one mcom_agree_mask; the
// lists' rows stay zero.  The array of the largest set and the mask must fit the card beside the rows.
uint8_t *agree_mask(Arena &A, const std::vector<Seg> &segs, uint64_t n_rows, int L, uint32_t *d_flag, int C)
{
	const uint64_t mb = (uint64_t)(L + 7) / 8;
	uint64_t most = 0;
	for (const Seg &s : segs) if (s.src.d_cid && s.ref_bases > most) most = s.ref_bases;
	{
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess || n_rows * mb + 9 * (most + 1) + ((size_t)64 << 20) > fr) {
			fprintf(stderr, "minicom gpu decoder: the mask of %llu rows and the coverage of %llu contig bases do not fit the card (%zu bytes free)\n", (unsigned long long)n_rows, (unsigned long long)most, fr);
			throw Refuse{"the agreement mask does not fit the card"};
		}
	}
	uint8_t *mask = A.alloc<uint8_t>(n_rows * mb);
	if (hipMemset(mask, 0, n_rows * mb + 16) != hipSuccess) throw Refuse{"memset failed"};
	uint8_t *cov = A.alloc<uint8_t>(most);
	for (const Seg &s : segs) {
		if (!s.src.d_cid || !s.n) continue;
		ok(A.ctx, mcom_agree_coverage(A.ctx, s.src.d_cid, s.src.d_pos, s.src.d_coff, s.src.n_contigs, s.n, L, s.ref_bases, cov, d_flag));
		ok(A.ctx, mcom_agree_mask(A.ctx, &s.src, s.n, L, s.d_dest, s.dest0, n_rows, cov, s.ref_bases, (uint32_t)C, mask, mb, d_flag));
		ok(A.ctx, mcom_sync(A.ctx));                                        // (the next set writes the same coverage array)
	}
	if (read_flag(A, d_flag)) throw Refuse{"a member's place leaves its contig"};
	return mask;
}

// the file(s): copy of piece i + 1 under the write of piece i
int write_files(Mode mode, Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L, const char *out_path1, const char *out_path2, uint64_t *n_out)
{
	const uint64_t row = (uint64_t)L + 1, table_bytes = n_rows * row;
	const double t0 = now_ms();
	uint8_t *pin[2] = {nullptr, nullptr};
	const int n_files = mode == PE ? 2 : 1;
	const char *paths[2] = {out_path1, out_path2};
	// everything that can be refused for want of memory is made before a file is opened: the plain route's two page-locked buffers and the
	// .gz route's sink, one for both files of a pair
	bool any_plain = false, any_gz = false;
	for (int fi = 0; fi < n_files; ++fi) (gz_path(paths[fi]) ? any_gz : any_plain) = true;
	for (int b = 0; b < 2 && any_plain; ++b) { void *p = nullptr; if (hipHostMalloc(&p, PIECE_BYTES, hipHostMallocDefault) != hipSuccess) throw Refuse{"no page-locked memory"}; A.pinned.push_back(p); pin[b] = (uint8_t*)p; }
	std::unique_ptr<GzSink> Z(any_gz ? new GzSink(A) : nullptr);
	bool wrote_ok = true;
	for (int fi = 0; fi < n_files && wrote_ok; ++fi) {
		const uint64_t first = mode == PE ? (uint64_t)fi * (uint64_t)half * row : 0, bytes = mode == PE ? (uint64_t)half * row : table_bytes;
		FILE *out = fopen(paths[fi], "wb");
		if (!out) { wrote_ok = false; break; }
		const uint64_t pieces = (bytes + PIECE_BYTES - 1) / PIECE_BYTES;
		auto piece_bytes = [&](uint64_t i) { const uint64_t at = i * PIECE_BYTES; return (size_t)(bytes - at < PIECE_BYTES ? bytes - at : PIECE_BYTES); };
		if (gz_path(paths[fi])) {                                              // each file of a pair starts afresh
			Z->carry = 0;
			for (uint64_t i = 0; i < pieces && wrote_ok; ++i) wrote_ok = Z->feed(table + first + i * PIECE_BYTES, piece_bytes(i), i + 1 == pieces, out);
			if (!pieces && wrote_ok) wrote_ok = Z->feed(nullptr, 0, true, out);
			if (fclose(out) != 0) wrote_ok = false;
			continue;
		}
		if (pieces && hipMemcpyAsync(pin[0], table + first, piece_bytes(0), hipMemcpyDeviceToHost, nullptr) != hipSuccess) wrote_ok = false;
		for (uint64_t i = 0; i < pieces && wrote_ok; ++i) {
			if (hipStreamSynchronize(nullptr) != hipSuccess) { wrote_ok = false; break; }
			if (i + 1 < pieces && hipMemcpyAsync(pin[(i + 1) & 1], table + first + (i + 1) * PIECE_BYTES, piece_bytes(i + 1), hipMemcpyDeviceToHost, nullptr) != hipSuccess) { wrote_ok = false; break; }
			const double tw = now_ms();
			if (fwrite(pin[i & 1], 1, piece_bytes(i), out) != piece_bytes(i)) wrote_ok = false;
			g_times[5] += now_ms() - tw;
		}
		(void)hipStreamSynchronize(nullptr);
		if (fclose(out) != 0) wrote_ok = false;
	}
	if (!wrote_ok) { for (int fi = 0; fi < n_files; ++fi) remove(paths[fi]); return -1; }
	g_times[4] = now_ms() - t0;
	if (n_out) *n_out = mode == PE ? (uint64_t)half : n_rows;
	return 0;
}

int guarded(Mode mode, const char *folder, const char *o1, const char *o2, uint64_t *n, int device)
{
	if (!folder || !o1 || (mode == PE && !o2)) return -1;
	try {
		return run(mode, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L) { return write_files(mode, A, table, n_rows, half, L, o1, o2, n); });
	} catch (...) { return -1; }   // no C++ exception crosses the C boundary
}

// ---- a -p -Q archive back to FASTQ: the third tail.  folder/qual.mcq is decoded on the device (mcom_qual_decode), the records
// `@<i+1>`, read, `+`, qualities are laid out by mcom_fastq_emit a piece at a time, the copy of piece i under the write of piece i - 1.
// With folder/name.mcn the names and '+' texts are decoded on the device as well and mcom_fastq_emit_named lays the records out.
// a `.mcq` member of the folder decoded on the device into rows `pitch` apart; it must state the reads' number and length.  flag: the
// command-line flag that makes such a member ("-Q" for qual.mcq, "-q" for rqual*.mcq): the refusals name the member and the flag
std::string g_why;                                      // the text of a refusal made of a member's name (Refuse carries a pointer)
[[noreturn]] void refuse_member(const std::string &why) { g_why = why; throw Refuse{g_why.c_str()}; }
// rng: the rows [rng->first, rng->first + rng->count) alone, to rows 0 .. (mcom_qual_decode_rows: the touched segments, no CRC of the whole)
uint8_t *load_quals(Arena &A, const char *folder, const char *member_name, const char *flag, uint64_t n_rows, int L, uint64_t pitch, const Window *rng = nullptr)
{
	const std::string name(member_name);
	std::vector<uint8_t> member;
	if (!slurp(std::string(folder) + "/" + name, member)) refuse_member("no " + name + ": not a " + flag + " archive");
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcom_qual_info(member.data(), member.size(), &qn, &qL) || qn != n_rows || (int)qL != L) refuse_member(name + " does not state the reads' number and length");
	const uint8_t *d_member = A.upload(member.data(), member.size());
	uint8_t *quals = A.alloc<uint8_t>((rng ? rng->count : n_rows) * pitch);
	if (rng ? mcom_qual_decode_rows(A.ctx, d_member, member.size(), rng->first, rng->count, quals, pitch, &qn, &qL) : mcom_qual_decode(A.ctx, d_member, member.size(), quals, pitch, n_rows, &qn, &qL)) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); refuse_member(name + " is refused"); }
	return quals;
}

// the two page-locked pieces and their device twins that the records travel through: made once per call, also where it writes two files
struct EmitBufs { uint8_t *pin[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr}; bool made = false; };

// a name text the caller has decoded already, with its record offsets on the device and on the host (the pair-in-input-order tail)
struct NamesReady { const uint8_t *d_names; const uint64_t *d_off; uint64_t bytes; const std::vector<uint64_t> *off; };

// quals_ready: the quality rows (pitch L) when the caller has decoded them already (the `minicom -q` tails: no names there, unless the
// caller hands them in as names_ready)
// rng (a record range, section 3.19): table and quality rows hold the n_rows = rng->count records from rng->first on; the side members
// state rng->n_records, the names are those of the whole archive and the records are numbered and named from `base` = rng->first
int write_fastq(Arena &A, const char *folder, const uint8_t *table, uint64_t n_rows, int L, const char *out_path, uint64_t *n_out, const uint8_t *quals_ready = nullptr, EmitBufs *shared = nullptr,
                const NamesReady *names_ready = nullptr, const Window *rng = nullptr)
{
	const uint64_t base = rng ? rng->first : 0, n_all = rng ? rng->n_records : n_rows;
	const uint8_t *quals = quals_ready ? quals_ready : load_quals(A, folder, "qual.mcq", "-Q", n_all, L, (uint64_t)L, rng);
	// folder/name.mcn (`minicom -N`, section 3.10): decoded on the device too; the records then carry its names and '+' texts
	std::vector<uint8_t> nmember;
	const bool own_names = !quals_ready && !names_ready && slurp(std::string(folder) + "/name.mcn", nmember), named = own_names || names_ready;
	const uint8_t *d_names = nullptr; const uint64_t *d_off = nullptr; uint64_t names_bytes = 0;
	std::vector<uint64_t> off_own;                                         // the record offsets of the name text, on the host: pieces are cut by them
	if (names_ready) { d_names = names_ready->d_names; d_off = names_ready->d_off; names_bytes = names_ready->bytes; }
	if (own_names) {
		uint64_t nn = 0;
		if (mcom_name_info(nmember.data(), nmember.size(), &nn, &names_bytes) || nn != n_all) throw Refuse{"name.mcn does not state the reads' number"};
		const uint8_t *d_nm = A.upload(nmember.data(), nmember.size());
		uint8_t *dn = A.alloc<uint8_t>(names_bytes); uint64_t *dof = A.alloc<uint64_t>(n_all + 1);
		if (mcom_name_decode(A.ctx, d_nm, nmember.size(), dn, names_bytes, &names_bytes, &nn, dof) || nn != n_all) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); throw Refuse{"name.mcn is refused"}; }
		d_names = dn; d_off = dof;
		off_own.resize(n_all + 1);
		if (hipMemcpy(off_own.data(), d_off, (n_all + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) throw Refuse{"download failed"};
	}
	const std::vector<uint64_t> &off = names_ready ? *names_ready->off : off_own;
	const double t0 = now_ms();
	const uint64_t rec_max = 2 * (uint64_t)L + 17, per_piece = PIECE_BYTES / rec_max;
	// where every piece begins: a fixed number of records without names; with names the most records whose bytes fit a piece (bisection
	// in the offset array: record r of a piece from `first` ends at (2 L + 4)(r + 1 - first) + off[r + 1] - off[first])
	if (!named && !per_piece) throw Refuse{"a record does not fit a piece"};
	std::vector<uint64_t> piece_at(1, 0);
	while (piece_at.back() < n_rows) {
		const uint64_t first = piece_at.back();
		uint64_t end = first + per_piece < n_rows ? first + per_piece : n_rows;
		if (named) {
			uint64_t lo = first + 1, hi = n_rows;                              // (one record always fits: at most 2 L + 4 + 512 bytes)
			while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if ((2 * (uint64_t)L + 4) * (mid - first) + off[base + mid] - off[base + first] <= PIECE_BYTES) lo = mid; else hi = mid - 1; }
			end = lo;
		}
		piece_at.push_back(end);
	}
	const uint64_t pieces = piece_at.size() - 1;
	EmitBufs own, &E = shared ? *shared : own;
	for (int b = 0; b < 2 && !E.made; ++b) {
		void *p = nullptr;
		if (hipHostMalloc(&p, PIECE_BYTES, hipHostMallocDefault) != hipSuccess) throw Refuse{"no page-locked memory"};
		A.pinned.push_back(p); E.pin[b] = (uint8_t*)p;
		E.d_out[b] = A.alloc<uint8_t>(pieces ? PIECE_BYTES : 1);
	}
	E.made = true;
	uint8_t *const *pin = E.pin, *const *d_out = E.d_out;
	struct Events { hipEvent_t e[2] = {nullptr, nullptr}; ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } arrived;   // piece i is in pin[i & 1]
	for (int b = 0; b < 2; ++b) if (hipEventCreateWithFlags(&arrived.e[b], hipEventDisableTiming) != hipSuccess) throw Refuse{"no events"};
	std::unique_ptr<GzSink> sink(gz_path(out_path) ? new GzSink(A) : nullptr);     // made before the file is opened: a refusal leaves no file
	FILE *out = fopen(out_path, "wb");
	if (!out) return -1;
	bool wrote_ok = true;
	uint64_t bytes[2] = {0, 0};
	if (sink) {
		GzSink &Z = *sink;
		for (uint64_t i = 0; i < pieces && wrote_ok; ++i) {
			const uint64_t first = piece_at[i], count = piece_at[i + 1] - first;
			const int rc = named ? mcom_fastq_emit_named(A.ctx, table + first * ((uint64_t)L + 1), (uint64_t)L + 1, quals + first * (uint64_t)L, (uint64_t)L, d_names, names_bytes, d_off + base + first, count,
			                                             (uint32_t)L, d_out[0], &bytes[0])
			                     : mcom_fastq_emit(A.ctx, table + first * ((uint64_t)L + 1), (uint64_t)L + 1, quals + first * (uint64_t)L, (uint64_t)L, base + first, count, (uint32_t)L, d_out[0], &bytes[0]);
			wrote_ok = !rc && bytes[0] <= PIECE_BYTES && Z.feed(d_out[0], (size_t)bytes[0], i + 1 == pieces, out);
		}
		if (!pieces && wrote_ok) wrote_ok = Z.feed(nullptr, 0, true, out);
		if (fclose(out) != 0) wrote_ok = false;
		if (!wrote_ok) { remove(out_path); return -1; }
		g_times[4] = now_ms() - t0;
		if (n_out) *n_out = n_rows;
		return 0;
	}
	for (uint64_t i = 0; i <= pieces && wrote_ok; ++i) {
		if (i < pieces) {
			const uint64_t first = piece_at[i], count = piece_at[i + 1] - first;
			const int rc = named ? mcom_fastq_emit_named(A.ctx, table + first * ((uint64_t)L + 1), (uint64_t)L + 1, quals + first * (uint64_t)L, (uint64_t)L, d_names, names_bytes, d_off + base + first, count,
			                                             (uint32_t)L, d_out[i & 1], &bytes[i & 1])
			                     : mcom_fastq_emit(A.ctx, table + first * ((uint64_t)L + 1), (uint64_t)L + 1, quals + first * (uint64_t)L, (uint64_t)L, base + first, count, (uint32_t)L, d_out[i & 1], &bytes[i & 1]);
			if (rc ||
			    bytes[i & 1] > PIECE_BYTES) { wrote_ok = false; break; }       // (synchronous on the context's stream: d_out[i & 1] is complete)
			if (hipMemcpyAsync(pin[i & 1], d_out[i & 1], bytes[i & 1], hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
			    hipEventRecord(arrived.e[i & 1], nullptr) != hipSuccess) { wrote_ok = false; break; }
		}
		if (i > 0) {
			if (hipEventSynchronize(arrived.e[(i - 1) & 1]) != hipSuccess) { wrote_ok = false; break; }   // piece i - 1 has arrived, whatever stream the context works on
			const double tw = now_ms();
			if (fwrite(pin[(i - 1) & 1], 1, bytes[(i - 1) & 1], out) != bytes[(i - 1) & 1]) wrote_ok = false;
			g_times[5] += now_ms() - tw;
		}
	}
	(void)hipStreamSynchronize(nullptr);
	if (fclose(out) != 0) wrote_ok = false;
	if (!wrote_ok) { remove(out_path); return -1; }
	g_times[4] = now_ms() - t0;
	if (n_out) *n_out = n_rows;
	return 0;
}

// name_1.mcn and name_2.mcn decoded on the device, name_2 against the decoded name_1 text; false: the archive has neither
struct PairNames { NamesReady r[2]; std::vector<uint64_t> off[2]; };
bool load_pair_names(Arena &A, const char *folder, uint64_t half, PairNames &P)
{
	std::vector<uint8_t> m[2];
	const bool has1 = slurp(std::string(folder) + "/name_1.mcn", m[0]), has2 = slurp(std::string(folder) + "/name_2.mcn", m[1]);
	if (has1 != has2) throw Refuse{"one of name_1.mcn and name_2.mcn is missing: name_2 is coded against name_1"};
	if (!has1) return false;
	uint8_t *d_text[2]; uint64_t bytes[2] = {0, 0};
	for (int k = 0; k < 2; ++k) {
		uint64_t nn = 0;
		if ((k ? mcom_name_info_mate(m[k].data(), m[k].size(), &nn, &bytes[k]) : mcom_name_info(m[k].data(), m[k].size(), &nn, &bytes[k])) || nn != half) throw Refuse{"a name member does not state the pairs' number"};
		const uint8_t *d_nm = A.upload(m[k].data(), m[k].size());
		d_text[k] = A.alloc<uint8_t>(bytes[k]);
		uint64_t *d_off = A.alloc<uint64_t>(half + 1);
		const int rc = k ? (mcom_name_decode_mate(A.ctx, d_nm, m[k].size(), d_text[0], bytes[0], d_text[1], bytes[1], &bytes[1], &nn) || mcom_name_text_offsets(A.ctx, d_text[1], bytes[1], half, d_off))
		                 : mcom_name_decode(A.ctx, d_nm, m[k].size(), d_text[0], bytes[0], &bytes[0], &nn, d_off);
		if (rc || nn != half) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); throw Refuse{"a name member is refused"}; }
		P.off[k].resize(half + 1);
		if (hipMemcpy(P.off[k].data(), d_off, (half + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) throw Refuse{"download failed"};
		P.r[k] = NamesReady{d_text[k], d_off, bytes[k], &P.off[k]};
	}
	return true;
}

// both files of a pair as FASTQ: the rows [0, half) of the table and the `half` behind them, the quality members qname1 / qname2 (made by
// `flag`) and -- with_pair_names -- name_1.mcn / name_2.mcn.  Every member is decoded before a file is opened, both files travel through
// the same two pieces, and neither is left when the second fails.  rng: as for write_fastq
int write_fastq_pair(Arena &A, const char *folder, const uint8_t *table, uint64_t half, int L, const char *o1, const char *o2, uint64_t *n_out, const char *qname1, const char *qname2, const char *flag,
                     bool with_pair_names, const Window *rng = nullptr)
{
	const uint64_t n_all = rng ? rng->n_records : half;
	const uint8_t *q1 = load_quals(A, folder, qname1, flag, n_all, L, (uint64_t)L, rng), *q2 = load_quals(A, folder, qname2, flag, n_all, L, (uint64_t)L, rng);
	PairNames P;
	const bool named = with_pair_names && load_pair_names(A, folder, n_all, P);
	EmitBufs bufs;
	if (write_fastq(A, folder, table, half, L, o1, n_out, q1, &bufs, named ? &P.r[0] : nullptr, rng)) return -1;
	int rc = -1;
	try { rc = write_fastq(A, folder, table + half * ((uint64_t)L + 1), half, L, o2, n_out, q2, &bufs, named ? &P.r[1] : nullptr, rng); } catch (...) { remove(o1); throw; }
	if (rc) remove(o1);
	return rc;
}

// ---- a ragged archive (`minicom -p -V`): the fourth tail.  The table holds the n_even reads of the modal length;
// folder/len.bin says where they stand among all records, odd.seq / odd.qual hold the lines of the others.  The side members are checked
// against one another by the rules the host decoder applies (mcom_ragged_load), the slots are made by mcom_ragged_index, and
// mcom_fastq_emit_ragged lays the records out a piece at a time: one read per line, or -- fastq -- four-line records.
struct RaggedDev {
	McomRaggedParts P;
	mcom_ragged_src S;
	std::vector<uint64_t> off;                              // record offsets of the name text, on the host (empty: no names)
};
// `minicom -V -A`: the full odd text rebuilt on the card from odd.aln, the residual (P.odd_seq as loaded) and the
// ref.bin images run() has uploaded, set after set into one packed text; P.odd_seq becomes the full text, which stays in HBM
const uint8_t *rebuild_odd(Arena &A, const char *folder, int L, McomRaggedParts &P)
{
	std::vector<uint8_t> member;
	if (!slurp(std::string(folder) + "/odd.aln", member)) refuse_member("cannot read odd.aln");
	std::vector<uint64_t> off(1, 0);
	for (uint8_t b : P.len) if ((int)b + 1 != L) off.push_back(off.back() + (uint64_t)b + 1);
	uint64_t bases = 0;
	for (const Arena::SetRef &s : A.set_refs) bases += s.bases;
	if (bases >= ((uint64_t)1 << 40)) refuse_member("the contigs hold 2^40 bases or more");
	const uint64_t words = (bases + 31) / 32 + 1;
	uint64_t *d_t = A.alloc<uint64_t>(words);
	if (hipMemset(d_t, 0, words * 8) != hipSuccess) throw Refuse{"memset failed"};
	uint64_t at = 0;
	for (const Arena::SetRef &s : A.set_refs) { ok(A.ctx, mcom_odd_text_append(A.ctx, d_t, words, at, s.d_ref, s.ref_bytes, s.bases)); at += s.bases; }
	const uint8_t *d_member = A.upload(member.data(), member.size()), *d_res = A.upload(P.odd_seq.data(), P.odd_seq.size());
	const uint64_t *d_off = A.upload(off.data(), off.size());
	uint8_t *d_out = A.alloc<uint8_t>(off.back());
	uint32_t flags = 0;
	if (mcom_odd_align_decode(A.ctx, d_member, member.size(), d_t, bases, d_res, P.odd_seq.size(), d_off, off.size() - 1, off.back(), d_out, &flags)) refuse_member(mcom_last_error(A.ctx));
	P.odd_seq.resize(off.back());
	if (off.back() && hipMemcpy(P.odd_seq.data(), d_out, off.back(), hipMemcpyDeviceToHost) != hipSuccess) throw Refuse{"download failed"};
	return d_out;
}

// the side members and, for fastq, the quality rows and the names, on the device; S ready for the emit call
void load_ragged(Arena &A, const char *folder, const uint8_t *table, uint64_t n_even, int L, bool fastq, RaggedDev &R)
{
	std::vector<uint8_t> qhead, nmember;
	const bool has_qual = slurp(std::string(folder) + "/qual.mcq", qhead), named = slurp(std::string(folder) + "/name.mcn", nmember);
	if (fastq && !has_qual) refuse_member("no qual.mcq: not a -Q archive");
	std::string why;
	const bool aligned = mcom_odd_align_present(folder);                      // then P.odd_seq is the residual, and the text is rebuilt below
	if (!mcom_ragged_load(folder, L, n_even, has_qual, R.P, why, !aligned)) refuse_member(why);
	uint64_t qn = 0, nn = 0, names_bytes = 0; uint32_t qL = 0;
	if (has_qual && (mcom_qual_info(qhead.data(), qhead.size(), &qn, &qL) || qn != n_even || (int)qL != L)) refuse_member("qual.mcq does not state the number and length of the reads of the modal length");
	if (named && (mcom_name_info(nmember.data(), nmember.size(), &nn, &names_bytes) || nn != R.P.n)) refuse_member("name.mcn does not state the records' number");
	mcom_ragged_src &S = R.S;
	memset(&S, 0, sizeof S);
	S.d_reads = table; S.read_pitch = (uint64_t)L + 1; S.n_even = n_even; S.L = (uint32_t)L; S.n = R.P.n;
	S.d_odd_seq = aligned ? rebuild_odd(A, folder, L, R.P) : A.upload(R.P.odd_seq.data(), R.P.odd_seq.size());
	S.odd_bytes = R.P.odd_seq.size();
	if (has_qual && R.P.odd_qual.size() != S.odd_bytes) refuse_member("the lengths of len.bin do not add up to the size of odd.qual");
	const uint8_t *d_len = A.upload(R.P.len.data(), R.P.len.size());
	uint64_t *d_slot = A.alloc<uint64_t>(R.P.n);
	uint64_t ne = 0, no = 0, ob = 0;
	ok(A.ctx, mcom_ragged_index(A.ctx, d_len, R.P.n, (uint32_t)L, d_slot, &ne, &no, &ob));
	if (ne != n_even || ob != S.odd_bytes) throw Refuse{"the slots do not match the side members"};
	S.d_len = d_len; S.d_slot = d_slot;
	if (!fastq) return;
	S.d_quals = load_quals(A, folder, "qual.mcq", "-Q", n_even, L, (uint64_t)L); S.qual_pitch = (uint64_t)L;
	S.d_odd_qual = A.upload(R.P.odd_qual.data(), R.P.odd_qual.size());
	if (named) {
		const uint8_t *d_nm = A.upload(nmember.data(), nmember.size());
		uint8_t *dn = A.alloc<uint8_t>(names_bytes); uint64_t *dof = A.alloc<uint64_t>(R.P.n + 1);
		if (mcom_name_decode(A.ctx, d_nm, nmember.size(), dn, names_bytes, &names_bytes, &nn, dof) || nn != R.P.n) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); throw Refuse{"name.mcn is refused"}; }
		S.d_names = dn; S.names_bytes = names_bytes; S.d_rec_off = dof;
		R.off.resize(R.P.n + 1);
		if (hipMemcpy(R.off.data(), dof, (R.P.n + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) throw Refuse{"download failed"};
	}
}

int write_ragged(Arena &A, const char *folder, const uint8_t *table, uint64_t n_even, int L, const char *out_path, uint64_t *n_out, bool fastq)
{
	RaggedDev R;
	load_ragged(A, folder, table, n_even, L, fastq, R);
	const uint64_t n = R.P.n;
	const double t0 = now_ms();
	// where every piece begins: the most records whose bytes fit a piece, counted on the host from len.bin and the name offsets
	std::vector<uint64_t> piece_at(1, 0);
	{
		uint64_t held = 0, digits = 1, next_pow = 10;
		for (uint64_t i = 0; i < n; ++i) {
			if (i + 1 >= next_pow) { ++digits; next_pow *= 10; }
			const uint64_t l = (uint64_t)R.P.len[i] + 1;
			uint64_t sz = !fastq ? l + 1 : R.off.empty() ? 2 * l + 6 + digits : 2 * l + 4 + (R.off[i + 1] >= R.off[i] ? R.off[i + 1] - R.off[i] : 0);
			if (sz > PIECE_BYTES) throw Refuse{"a record does not fit a piece"};
			if (held + sz > PIECE_BYTES) { piece_at.push_back(i); held = 0; }
			held += sz;
		}
		if (n) piece_at.push_back(n);
	}
	const uint64_t pieces = piece_at.size() - 1;
	void *p = nullptr;
	if (hipHostMalloc(&p, PIECE_BYTES, hipHostMallocDefault) != hipSuccess) throw Refuse{"no page-locked memory"};
	A.pinned.push_back(p);
	uint8_t *pin = (uint8_t*)p, *d_out = A.alloc<uint8_t>(PIECE_BYTES);
	std::unique_ptr<GzSink> sink(gz_path(out_path) ? new GzSink(A) : nullptr);     // made before the file is opened: a refusal leaves no file
	FILE *out = fopen(out_path, "wb");
	if (!out) return -1;
	bool wrote_ok = true;
	for (uint64_t i = 0; i < pieces && wrote_ok; ++i) {
		uint64_t bytes = 0;
		if (mcom_fastq_emit_ragged(A.ctx, &R.S, piece_at[i], piece_at[i + 1] - piece_at[i], d_out, PIECE_BYTES, &bytes)) { fprintf(stderr, "minicom gpu decoder: %s\n", mcom_last_error(A.ctx)); wrote_ok = false; break; }
		if (sink) wrote_ok = sink->feed(d_out, (size_t)bytes, i + 1 == pieces, out);
		else {
			wrote_ok = hipMemcpy(pin, d_out, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess;
			const double tw = now_ms();
			wrote_ok = wrote_ok && fwrite(pin, 1, (size_t)bytes, out) == bytes;
			g_times[5] += now_ms() - tw;
		}
	}
	if (sink && !pieces && wrote_ok) wrote_ok = sink->feed(nullptr, 0, true, out);
	if (fclose(out) != 0) wrote_ok = false;
	if (!wrote_ok) { remove(out_path); return -1; }
	g_times[4] = now_ms() - t0;
	if (n_out) *n_out = n;
	return 0;
}

// ---- verification: the rows of phase B against the reads of the FASTQ file(s), both in HBM (csrc/verify.hip) ----
// Side a is the input, side b the archive: `missing` are reads of the input that the archive does not give back.
int compare_rows(Mode mode, Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L, const uint8_t *d_in, uint64_t n_in, int L_in, mcomh_verify_report *rep)
{
	if (n_in && L_in != L) { fprintf(stderr, "minicom verify: the reads of the FASTQ are %d long, those of the archive %d\n", L_in, L); return -1; }
	mcom_verify_table a, b;
	a.d_rows = d_in; a.pitch = (uint64_t)L; a.n = mode == PE ? n_in / 2 : n_in; a.d_mates = mode == PE ? d_in + a.n * (uint64_t)L : nullptr;
	b.d_rows = table; b.pitch = (uint64_t)L + 1; b.n = mode == PE ? half : n_rows; b.d_mates = mode == PE ? table + half * ((uint64_t)L + 1) : nullptr;
	if (mode != ORDER) {
		const uint64_t room = mcom_verify_room(a.n, b.n);
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess || room > fr) {
			fprintf(stderr, "minicom verify: the card has no room: %llu bytes for the reads of the FASTQ, %llu for the archive's rows and %llu for the records and their sort are needed, %zu of the last are free\n",
			        (unsigned long long)(n_in * (uint64_t)L), (unsigned long long)(n_rows * ((uint64_t)L + 1)), (unsigned long long)room, fr);
			return -1;
		}
	}
	const double t0 = now_ms();
	mcom_verify_report r;
	(void)hipEventRecord(A.ev[0], nullptr);
	ok(A.ctx, mode == ORDER ? mcom_verify_ordered(A.ctx, &a, &b, L, &r) : mcom_verify_multiset(A.ctx, &a, &b, L, &r));
	(void)hipEventRecord(A.ev[1], nullptr);
	(void)hipEventSynchronize(A.ev[1]);
	{ float ms = 0; if (hipEventElapsedTime(&ms, A.ev[0], A.ev[1]) == hipSuccess) rep->times_ms[6] = ms; }
	rep->times_ms[3] = now_ms() - t0;
	rep->identical = r.identical; rep->n_input = r.n_a; rep->n_archive = r.n_b;
	rep->missing = r.missing; rep->extra = r.extra; rep->differing = r.differing; rep->first_diff = r.first_diff; rep->exact_runs = r.exact_runs;
	rep->n_missing_ex = r.n_missing_ex; rep->n_extra_ex = r.n_extra_ex;
	memcpy(rep->missing_ex, r.missing_ex, sizeof(r.missing_ex)); memcpy(rep->extra_ex, r.extra_ex, sizeof(r.extra_ex));
	return 0;
}

int verify(const char *folder, int mode, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	const double t_begin = now_ms();
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
			fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev);
			return -1;
		}
	}
	struct Reads { uint8_t *d = nullptr; ~Reads() { mcomh_device_free(d); } } in;
	size_t n_in = 0; int L_in = 0;
	char err[256] = "";
	const int rc = mode == PE ? mcomh_fastq_pair_to_device(fastq1, fastq2, device, &L_in, 0, &in.d, &n_in, err, sizeof(err))
	                          : mcomh_fastq_to_device(fastq1, device, &L_in, 0, &in.d, &n_in, err, sizeof(err));
	if (rc) { fprintf(stderr, "minicom verify: cannot read %s%s%s: %s\n", fastq1, mode == PE ? " and " : "", mode == PE ? fastq2 : "", err[0] ? err : "not a FASTQ / FASTA file of reads of one length"); return -1; }
	const double ingest = now_ms() - t_begin;
	const int rr = run((Mode)mode, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L) {
		return compare_rows((Mode)mode, A, table, n_rows, half, L, in.d, (uint64_t)n_in, L_in, rep);
	});
	if (rr) return -1;
	rep->mode = mode;
	rep->times_ms[0] = ingest; rep->times_ms[1] = g_times[1]; rep->times_ms[2] = g_times[2]; rep->times_ms[5] = g_times[0]; rep->times_ms[7] = g_times[3];
	rep->times_ms[4] = now_ms() - t_begin;
	return 0;
}

// ---- `minicom -q -a`: the records of a default-mode archive against those of the file UNDER THE MASK.  The archive
// does not say which record of the file a row was, and the mask row belongs to the archive's row, so "identical" means: there is a
// one-to-one assignment of the file's records to the archive's rows such that every record has its row's read and, sent through its row's
// mask (then through qual_lossy.txt's transform), its row's quality values.  Rows and records are grouped by read (a sort of either side);
// a group of one is compared directly, a larger group is a bipartite matching (augmenting paths: exact, and a group is a handful of
// records unless the file repeats a read thousands of times).  The rows, the mask and the quality rows are made on the device as ever;
// the matching itself is host code over their downloaded bytes.
struct AgreeRecords {
	int L = 0; uint32_t Q = 0; bool lossy = false; mcomh_qual_lossy_spec spec;
	std::vector<uint8_t> a_reads, a_quals, mask, f_reads, f_quals;          // archive: pitch L + 1, L, (L + 7) / 8; file: pitch L
	uint64_t na = 0, nf = 0;
	const uint8_t *aread(uint64_t j) const { return a_reads.data() + j * ((size_t)L + 1); }
	const uint8_t *fread_(uint64_t k) const { return f_reads.data() + k * (size_t)L; }
	// does record k of the file, sent through row j's mask, give row j's quality values?
	bool fits(uint64_t k, uint64_t j) const
	{
		uint8_t tmp[256];
		memcpy(tmp, f_quals.data() + k * (size_t)L, (size_t)L);
		const uint8_t *m = mask.data() + j * (size_t)((L + 7) / 8);
		for (int i = 0; i < L; ++i) if ((m[i >> 3] >> (i & 7)) & 1u) tmp[i] = (uint8_t)(33 + Q);
		if (lossy && mcomh_qual_transform(tmp, 1, (uint32_t)L, (uint64_t)L, &spec, nullptr)) return false;
		return !memcmp(tmp, a_quals.data() + j * (size_t)L, (size_t)L);
	}
	void compare(mcomh_verify_report *rep) const
	{
		std::vector<uint64_t> ia(na), jf(nf);
		for (uint64_t i = 0; i < na; ++i) ia[i] = i;
		for (uint64_t i = 0; i < nf; ++i) jf[i] = i;
		std::sort(ia.begin(), ia.end(), [&](uint64_t x, uint64_t y) { const int c = memcmp(aread(x), aread(y), (size_t)L); return c < 0 || (c == 0 && x < y); });
		std::sort(jf.begin(), jf.end(), [&](uint64_t x, uint64_t y) { const int c = memcmp(fread_(x), fread_(y), (size_t)L); return c < 0 || (c == 0 && x < y); });
		uint64_t missing = 0, extra = 0, runs = 0;
		auto miss = [&](uint64_t k) { if (rep->n_missing_ex < 8) rep->missing_ex[rep->n_missing_ex++] = k; ++missing; };
		auto over = [&](uint64_t j) { if (rep->n_extra_ex < 8) rep->extra_ex[rep->n_extra_ex++] = j; ++extra; };
		uint64_t a = 0, f = 0;
		while (a < na || f < nf) {
			const int c = a >= na ? 1 : f >= nf ? -1 : memcmp(aread(ia[a]), fread_(jf[f]), (size_t)L);
			if (c < 0) { over(ia[a++]); continue; }
			if (c > 0) { miss(jf[f++]); continue; }
			uint64_t a1 = a + 1, f1 = f + 1;
			while (a1 < na && !memcmp(aread(ia[a1]), aread(ia[a]), (size_t)L)) ++a1;
			while (f1 < nf && !memcmp(fread_(jf[f1]), fread_(jf[f]), (size_t)L)) ++f1;
			const size_t ga = (size_t)(a1 - a), gf = (size_t)(f1 - f);
			if (ga > 1 || gf > 1) ++runs;
			// row_of[x]: the file record (index into the group) matched to archive row x of the group, or -1
			std::vector<long> row_of(ga, -1);
			std::vector<char> seen;
			std::function<bool(size_t)> place = [&](size_t y) {                   // an augmenting path from file record y
				for (size_t x = 0; x < ga; ++x) {
					if (seen[x] || !fits(jf[f + y], ia[a + x])) continue;
					seen[x] = 1;
					if (row_of[x] < 0 || place((size_t)row_of[x])) { row_of[x] = (long)y; return true; }
				}
				return false;
			};
			for (size_t y = 0; y < gf; ++y) { seen.assign(ga, 0); if (!place(y)) miss(jf[f + y]); }
			for (size_t x = 0; x < ga; ++x) if (row_of[x] < 0) over(ia[a + x]);
			a = a1; f = f1;
		}
		rep->n_input = nf; rep->n_archive = na; rep->missing = missing; rep->extra = extra; rep->exact_runs = runs;
		rep->identical = missing == 0 && extra == 0 && na == nf;
	}
};

// records with their quality lines (`minicom -q`): side a = the reads and quality rows of the FASTQ file(s) at pitch L, side b = the decoder's
// image and the rows of rqual*.mcq decoded beside it at pitch L + 1; 2 parts in the default mode, 4 in the paired-end mode
int verify_records(const char *folder, int mode, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	const double t_begin = now_ms();
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev); return -1; }
	}
	const std::string dir(folder);
	{
		FILE *f = fopen((dir + "/allA.ids.bin").c_str(), "rb");
		if (f) { fclose(f); fprintf(stderr, "minicom verify: %s is a -p archive\n", folder); return -1; }
		f = fopen((dir + "/file.bin.sp").c_str(), "rb");
		if (f) fclose(f);
		if ((f != nullptr) != (mode == PE)) { fprintf(stderr, "minicom verify: %s is %sa paired-end archive\n", folder, f ? "" : "not "); return -1; }
	}
	// an archive made with -a (qual_agree.txt, section 3.17): the single-file archive is compared under its mask; a paired one has none
	uint32_t agree_Q = 0, agree_C = 0;
	const int have_agree = mcomh_qual_agree_marker(folder, &agree_Q, &agree_C);
	if (have_agree < 0) { fprintf(stderr, "minicom verify: %s/qual_agree.txt does not hold `Q C` (0 .. 93, 1 .. 255) and a newline\n", folder); return -1; }
	if (have_agree && mode == PE) { fprintf(stderr, "minicom verify: %s carries qual_agree.txt, and a paired-end archive of the default mode has no agreement mask\n", folder); return -1; }
	struct Dev { uint8_t *d = nullptr; ~Dev() { mcomh_device_free(d); } } in, qin[2];
	size_t n_in = 0, nq[2] = {0, 0}; int L_in = 0;
	char err[320] = "";
	const int rc = mode == PE ? mcomh_fastq_pair_to_device(fastq1, fastq2, device, &L_in, 0, &in.d, &n_in, err, sizeof(err))
	                          : mcomh_fastq_to_device(fastq1, device, &L_in, 0, &in.d, &n_in, err, sizeof(err));
	if (rc) { fprintf(stderr, "minicom verify: cannot read %s%s%s: %s\n", fastq1, mode == PE ? " and " : "", mode == PE ? fastq2 : "", err[0] ? err : "not a FASTQ file of reads of one length"); return -1; }
	const char *fq[2] = {fastq1, fastq2};
	const int n_files = mode == PE ? 2 : 1;
	const size_t n_rec = mode == PE ? n_in / 2 : n_in;
	for (int k = 0; k < n_files; ++k) {
		if (L_in < 1 || mcomh_fastq_qualities_to_device(fq[k], device, L_in, 0, &qin[k].d, &nq[k], err, sizeof(err)) || nq[k] != n_rec) {
			fprintf(stderr, "minicom verify: cannot read the qualities of %s: %s\n", fq[k], err[0] ? err : "another number of records than reads"); return -1;
		}
		// an archive made with -b holds T(file): row-local, so it commutes with the order (under -a it follows the mask, row by row: AgreeRecords)
		if (!have_agree && mcom_qual_lossy_apply_marker(folder, device, qin[k].d, nq[k], L_in)) return -1;
	}
	const double ingest = now_ms() - t_begin;
	const uint8_t *d_mask = nullptr;
	const Between between = [&](Arena &A, const std::vector<Seg> &segs, uint64_t n_rows, int L, uint32_t *d_flag) { d_mask = agree_mask(A, segs, n_rows, L, d_flag, (int)agree_C); };
	const int rr = run((Mode)mode, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t half, int L) {
		if (n_in && L_in != L) { fprintf(stderr, "minicom verify: the reads of the FASTQ are %d long, those of the archive %d\n", L_in, L); return -1; }
		const uint64_t row = (uint64_t)L + 1, nb = mode == PE ? half : n_rows;
		if (have_agree) {
			AgreeRecords R;
			R.L = L; R.Q = agree_Q; R.na = n_rows; R.nf = n_rec;
			const int lm = mcomh_qual_lossy_marker(folder, &R.spec, nullptr, 0);
			if (lm < 0) { fprintf(stderr, "minicom verify: %s/qual_lossy.txt does not hold a lossy spec (ill8, thr:T:LO:HI, pblock:P) and a newline\n", folder); return -1; }
			R.lossy = lm == 1;
			const uint8_t *d_q = load_quals(A, folder, "rqual.mcq", "-q", n_rows, L, (uint64_t)L);
			const size_t mb = (size_t)(L + 7) / 8;
			R.a_reads.resize((size_t)n_rows * row + 1); R.a_quals.resize((size_t)n_rows * L + 1); R.mask.resize((size_t)n_rows * mb + 1);
			R.f_reads.resize(n_rec * (size_t)L + 1); R.f_quals.resize(n_rec * (size_t)L + 1);
			if ((n_rows && (hipMemcpy(R.a_reads.data(), table, (size_t)n_rows * row, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(R.a_quals.data(), d_q, (size_t)n_rows * L, hipMemcpyDeviceToHost) != hipSuccess ||
			                hipMemcpy(R.mask.data(), d_mask, (size_t)n_rows * mb, hipMemcpyDeviceToHost) != hipSuccess)) ||
			    (n_rec && (hipMemcpy(R.f_reads.data(), in.d, n_rec * (size_t)L, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(R.f_quals.data(), qin[0].d, n_rec * (size_t)L, hipMemcpyDeviceToHost) != hipSuccess))) {
				fprintf(stderr, "minicom verify: download failed\n"); return -1;
			}
			const double t0 = now_ms();
			R.compare(rep);
			rep->times_ms[3] = now_ms() - t0;
			return 0;
		}
		mcom_verify_parts a, b;
		memset(&a, 0, sizeof a); memset(&b, 0, sizeof b);
		a.pitch = (uint64_t)L; a.n = n_rec; b.pitch = row; b.n = nb;
		if (mode == PE) {
			a.n_parts = b.n_parts = 4;
			a.d_part[0] = in.d; a.d_part[1] = in.d + n_rec * (uint64_t)L; a.d_part[2] = qin[0].d; a.d_part[3] = qin[1].d;
			b.d_part[0] = table; b.d_part[1] = table + half * row;
			b.d_part[2] = load_quals(A, folder, "rqual_1.mcq", "-q", nb, L, row); b.d_part[3] = load_quals(A, folder, "rqual_2.mcq", "-q", nb, L, row);
		} else {
			a.n_parts = b.n_parts = 2;
			a.d_part[0] = in.d; a.d_part[1] = qin[0].d;
			b.d_part[0] = table; b.d_part[1] = load_quals(A, folder, "rqual.mcq", "-q", nb, L, row);
		}
		const uint64_t room = mcom_verify_room(a.n, b.n);
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess || room > fr) { fprintf(stderr, "minicom verify: the card has no room for the records and their sort (%llu bytes needed, %zu free)\n", (unsigned long long)room, fr); return -1; }
		const double t0 = now_ms();
		mcom_verify_report r;
		ok(A.ctx, mcom_verify_multiset_parts(A.ctx, &a, &b, L, &r));
		rep->times_ms[3] = now_ms() - t0;
		rep->identical = r.identical; rep->n_input = r.n_a; rep->n_archive = r.n_b;
		rep->missing = r.missing; rep->extra = r.extra; rep->differing = r.differing; rep->first_diff = r.first_diff; rep->exact_runs = r.exact_runs;
		rep->n_missing_ex = r.n_missing_ex; rep->n_extra_ex = r.n_extra_ex;
		memcpy(rep->missing_ex, r.missing_ex, sizeof(r.missing_ex)); memcpy(rep->extra_ex, r.extra_ex, sizeof(r.extra_ex));
		return 0;
	}, have_agree ? &between : nullptr);
	if (rr) return -1;
	rep->mode = mode;
	rep->times_ms[0] = ingest; rep->times_ms[1] = g_times[1]; rep->times_ms[2] = g_times[2]; rep->times_ms[5] = g_times[0]; rep->times_ms[7] = g_times[3];
	rep->times_ms[4] = now_ms() - t_begin;
	return 0;
}

} // namespace

extern "C" int mcomh_decompress_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device) { return guarded(DEFAULT, folder, out_path, nullptr, n_reads, device); }
extern "C" int mcomh_decompress_order_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device)
{
	if (folder && out_path && mcom_ragged_present(folder)) {                   // `minicom -p -V`: the records in input order, one read per line
		try {
			return run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) { return write_ragged(A, folder, table, n_rows, L, out_path, n_reads, false); });
		} catch (...) { return -1; }
	}
	return guarded(ORDER, folder, out_path, nullptr, n_reads, device);
}
extern "C" int mcomh_decompress_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device) { return guarded(PE, folder, out_path1, out_path2, n_pairs, device); }
extern "C" int mcomh_decompress_fastq_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device)
{
	if (!folder || !out_path) return -1;
	try {
		const bool ragged = mcom_ragged_present(folder);                        // `minicom -p -V -Q`: the fourth tail
		return run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			return ragged ? write_ragged(A, folder, table, n_rows, L, out_path, n_reads, true) : write_fastq(A, folder, table, n_rows, L, out_path, n_reads);
		});
	} catch (...) { return -1; }
}
// ---- `minicom -q` archives: the default / paired-end decoder's rows, the quality rows of rqual*.mcq (stored in
// the archive's own order) beside them, the records laid out as above.  What the host routes of mcom_decompress.cpp refuse is refused.
extern "C" int mcomh_decompress_fastq_reordered_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device)
{
	if (!folder || !out_path) return -1;
	if (exists(std::string(folder) + "/allA.ids.bin") || exists(std::string(folder) + "/file.bin.sp")) { fprintf(stderr, "minicom gpu decoder: %s is a -p or a paired-end archive\n", folder); return -1; }
	try {
		return run(DEFAULT, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			const uint8_t *q = load_quals(A, folder, "rqual.mcq", "-q", n_rows, L, (uint64_t)L);
			return write_fastq(A, folder, table, n_rows, L, out_path, n_reads, q);
		});
	} catch (...) { return -1; }
}
extern "C" int mcomh_decompress_fastq_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	if (exists(std::string(folder) + "/allA.ids.bin")) { fprintf(stderr, "minicom gpu decoder: %s is a -p archive\n", folder); return -1; }
	try {
		return run(PE, folder, device, [&](Arena &A, const uint8_t *table, uint64_t, uint64_t half, int L) {
			return write_fastq_pair(A, folder, table, half, L, out_path1, out_path2, n_pairs, "rqual_1.mcq", "rqual_2.mcq", "-q", false);
		});
	} catch (...) { return -1; }
}
// ---- a pair kept in input order (`minicom -1 -2 -p [-Q [-N]]`): the -p decoder's 2 n rows, [0, n) the first file and
// [n, 2 n) the second; folder/pe_order.txt must state n.  What the host routes of mcom_decompress.cpp refuse is refused, neither file is left.
extern "C" int mcomh_decompress_order_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	try {
		return run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			const uint64_t half = pairs_of(folder, n_rows);
			return write_files(PE, A, table, n_rows, half, L, out_path1, out_path2, n_pairs);
		});
	} catch (...) { return -1; }
}
extern "C" int mcomh_decompress_fastq_order_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	try {
		return run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			return write_fastq_pair(A, folder, table, pairs_of(folder, n_rows), L, out_path1, out_path2, n_pairs, "qual_1.mcq", "qual_2.mcq", "-Q", true);
		});
	} catch (...) { return -1; }
}
// ---- a record range of a -p archive (`minicom -d -R`; the host twin and the refusals that need no decoding:
// mcom_decompress.cpp).  run() makes the window's rows; the tails are the plain file(s), the FASTQ emit in pieces and the BGZF sink of
// `.gz` paths over them, with `first` carried into the names.  Every side member is decoded before a file is opened.
int mcom_range_gpu(const char *folder, const char *o1, const char *o2, uint64_t first, uint64_t count, uint64_t *n_written, int device, bool pair, bool fastq)
{
	try {
		Window W{first, count, pair};
		return run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			const uint64_t cnt = W.count;                                          // (clipped by run(); n_rows = cnt, or 2 cnt for a pair)
			if (!fastq) return write_files(pair ? PE : ORDER, A, table, n_rows, cnt, L, o1, o2, n_written);
			if (!pair) return write_fastq(A, folder, table, cnt, L, o1, n_written, nullptr, nullptr, nullptr, &W);
			return write_fastq_pair(A, folder, table, cnt, L, o1, o2, n_written, "qual_1.mcq", "qual_2.mcq", "-Q", true, &W);
		}, nullptr, &W);
	} catch (...) { return -1; }   // no C++ exception crosses the C boundary
}

// the reads of such an archive against the two FASTQ files, line against line over both files: the report's mode is 1
extern "C" int mcomh_verify_order_pe_reads_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	if (!folder || !fastq1 || !fastq2 || !rep) return -1;
	memset(rep, 0, sizeof(*rep));
	try {
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev); return -1; }
		struct Reads { uint8_t *d = nullptr; ~Reads() { mcomh_device_free(d); } } in;
		size_t n_in = 0; int L_in = 0;
		char err[256] = "";
		if (mcomh_fastq_pair_to_device(fastq1, fastq2, device, &L_in, 0, &in.d, &n_in, err, sizeof(err))) { fprintf(stderr, "minicom verify: cannot read %s and %s: %s\n", fastq1, fastq2, err[0] ? err : "not two FASTQ files of as many reads of one length"); return -1; }
		const int rr = run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			(void)pairs_of(folder, n_rows);
			return compare_rows(ORDER, A, table, n_rows, 0, L, in.d, (uint64_t)n_in, L_in, rep);
		});
		if (rr) return -1;
		rep->mode = 1;
		return 0;
	} catch (...) { return -1; }
}
// ---- verification of a `minicom -q` archive: records of (read, quality) or (read 1, read 2, quality 1, quality 2) as multisets ----
extern "C" int mcomh_verify_records_gpu(const char *folder, int mode, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	if (!folder || !fastq1 || !rep || (mode != 0 && mode != 2) || (mode == PE) != (fastq2 != nullptr)) {
		fprintf(stderr, "minicom verify: bad arguments (a folder, mode 0 default | 2 paired end, one FASTQ file, and the mates' file with mode 2 only)\n");
		return -1;
	}
	memset(rep, 0, sizeof(*rep));
	try { return verify_records(folder, mode, fastq1, fastq2, device, rep); } catch (...) { return -1; }
}
// ---- `minicom -d -c` for a ragged archive: the file is split again -- its lengths, then its sequence lines and, when
// the archive keeps them, its quality lines -- and every part is set against what the archive gives back: len.bin and the odd texts byte for
// byte on the host (they are read from the folder as they are), the even reads and the even quality rows by mcom_verify_ordered in HBM.
// Exact.  rep[0 .. 4]: len.bin, even reads, even quality rows, odd.seq, odd.qual; for the byte-wise parts `differing` counts bytes and
// first_diff is the first record whose byte differs (~0: none, or a byte behind the shorter side's end).
namespace {
void bytes_report(const std::vector<uint8_t> &a, const std::vector<uint8_t> &b, mcomh_verify_report *r, const std::vector<uint8_t> *len_of_a, int L)
{
	memset(r, 0, sizeof *r);
	r->mode = 1; r->n_input = a.size(); r->n_archive = b.size(); r->first_diff = ~(uint64_t)0;
	const size_t m = a.size() < b.size() ? a.size() : b.size();
	size_t first = m;
	for (size_t i = 0; i < m; ++i) if (a[i] != b[i]) { if (!r->differing) first = i; ++r->differing; }
	r->identical = !r->differing && a.size() == b.size();
	if (r->identical) return;
	if (!len_of_a) { r->first_diff = first; return; }                       // len.bin: byte r is record r
	uint64_t at = 0;                                                       // an odd text: the odd record of the input that holds byte `first`
	for (size_t rec = 0; rec < len_of_a->size(); ++rec) {
		const uint64_t l = (uint64_t)(*len_of_a)[rec] + 1;
		if ((int)l == L) continue;
		if (first < at + l) { r->first_diff = rec; return; }
		at += l;
	}
}
void rows_report(const mcom_verify_report &r, mcomh_verify_report *rep)
{
	memset(rep, 0, sizeof *rep);
	rep->mode = 1;
	rep->identical = r.identical; rep->n_input = r.n_a; rep->n_archive = r.n_b;
	rep->missing = r.missing; rep->extra = r.extra; rep->differing = r.differing; rep->first_diff = r.first_diff; rep->exact_runs = r.exact_runs;
}
}  // namespace

extern "C" int mcomh_verify_ragged_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report rep[5], int present[5])
{
	if (!folder || !fastq || !rep || !present) return -1;
	for (int k = 0; k < 5; ++k) present[k] = 0;
	try {
		const double t_begin = now_ms();
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { fprintf(stderr, "minicom verify: no GPU %d (%d visible); there is no host route\n", device, n_dev); return -1; }
		if (!mcom_ragged_present(folder)) { fprintf(stderr, "minicom verify: %s has no len.bin: not an archive made with -V\n", folder); return -1; }
		const std::string dir(folder), tmp_len = dir + "/verify_len.tmp";
		struct Tmp { std::string p; ~Tmp() { remove(p.c_str()); } } tmp{tmp_len};
		char err[320] = "";
		uint64_t n_in = 0, n_odd_in = 0, ne_in = 0, ne_q = 0; int L_in = 0;
		if (mcomh_fastq_lengths_file(fastq, device, 0, tmp_len.c_str(), &n_in, &L_in, &n_odd_in, err, sizeof err)) { fprintf(stderr, "minicom verify: cannot read %s: %s\n", fastq, err); return -1; }
		std::vector<uint8_t> len_in, odd_seq_in, odd_qual_in;
		if (!slurp(tmp_len, len_in)) return -1;
		const bool has_qual = exists(dir + "/qual.mcq");
		struct Dev { uint8_t *d = nullptr; ~Dev() { mcomh_device_free(d); } } in, qin;
		if (mcom_ragged_split_to_device(fastq, device, 1, L_in, tmp_len.c_str(), &in.d, odd_seq_in, &ne_in, err, sizeof err) ||
		    (has_qual && mcom_ragged_split_to_device(fastq, device, 3, L_in, tmp_len.c_str(), &qin.d, odd_qual_in, &ne_q, err, sizeof err))) {
			fprintf(stderr, "minicom verify: cannot read %s: %s\n", fastq, err); return -1;
		}
		const double ingest = now_ms() - t_begin;
		const int rr = run(ORDER, folder, device, [&](Arena &A, const uint8_t *table, uint64_t n_rows, uint64_t, int L) {
			RaggedDev R;
			load_ragged(A, folder, table, n_rows, L, has_qual, R);
			bytes_report(len_in, R.P.len, &rep[0], nullptr, L_in); present[0] = 1;
			bytes_report(odd_seq_in, R.P.odd_seq, &rep[3], &len_in, L_in); present[3] = 1;
			if (has_qual) { bytes_report(odd_qual_in, R.P.odd_qual, &rep[4], &len_in, L_in); present[4] = 1; }
			if (L_in != L) return 0;                                           // another modal length: len.bin differs, and rows of two widths are not compared
			mcom_verify_table a, b;
			mcom_verify_report r;
			a.d_rows = in.d; a.pitch = (uint64_t)L; a.n = ne_in; a.d_mates = nullptr;
			b.d_rows = table; b.pitch = (uint64_t)L + 1; b.n = n_rows; b.d_mates = nullptr;
			ok(A.ctx, mcom_verify_ordered(A.ctx, &a, &b, L, &r));
			rows_report(r, &rep[1]); present[1] = 1;
			if (has_qual) {
				a.d_rows = qin.d; a.n = ne_q;
				b.d_rows = R.S.d_quals; b.pitch = (uint64_t)L;
				ok(A.ctx, mcom_verify_ordered(A.ctx, &a, &b, L, &r));
				rows_report(r, &rep[2]); present[2] = 1;
			}
			return 0;
		});
		if (rr) return -1;
		rep[0].times_ms[0] = ingest; rep[0].times_ms[4] = now_ms() - t_begin;
		return 0;
	} catch (...) { return -1; }
}

// ---- the agreement mask of a folder (`minicom -a Q[:C]`; mcomh_agree_mask of mcom_agree.cpp): phases A and B as
// ever -- an archive the decoder refuses has no mask -- then agree_mask() between B and C, and the mask comes back to the host as the tail.
int mcom_agree_mask_gpu(const char *folder, bool order, int C, int device, std::vector<uint8_t> &mask, uint64_t *n_rows_out, int *L_out)
{
	if (!folder || C < 1 || C > 255) return -1;
	try {
		const uint8_t *d_mask = nullptr;
		const Between between = [&](Arena &A, const std::vector<Seg> &segs, uint64_t n_rows, int L, uint32_t *d_flag) { d_mask = agree_mask(A, segs, n_rows, L, d_flag, C); };
		return run(order ? ORDER : DEFAULT, folder, device, [&](Arena &, const uint8_t *, uint64_t n_rows, uint64_t, int L) {
			const size_t bytes = (size_t)n_rows * (size_t)((L + 7) / 8);
			mask.resize(bytes);
			if (bytes && hipMemcpy(mask.data(), d_mask, bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
			if (n_rows_out) *n_rows_out = n_rows;
			if (L_out) *L_out = L;
			return 0;
		}, &between);
	} catch (...) { return -1; }   // no C++ exception crosses the C boundary
}

extern "C" int mcomh_test_decoder_piece_bytes(size_t bytes)
{
	if (bytes && bytes < 4096) return -1;
	PIECE_BYTES = bytes ? bytes : (size_t)64 << 20;
	return 0;
}
extern "C" void mcomh_decompress_gpu_times(double *ms8) { if (ms8) memcpy(ms8, g_times, sizeof(g_times)); }
extern "C" int mcomh_verify_gpu(const char *folder, int mode, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep)
{
	if (!folder || !fastq1 || !rep || mode < 0 || mode > 2 || (mode == PE) != (fastq2 != nullptr)) {
		fprintf(stderr, "minicom verify: bad arguments (a folder, mode 0 default | 1 -p | 2 paired end, one FASTQ file, and the mates' file with mode 2 only)\n");
		return -1;
	}
	memset(rep, 0, sizeof(*rep));
	try { return verify(folder, mode, fastq1, fastq2, device, rep); } catch (...) { return -1; }
}
