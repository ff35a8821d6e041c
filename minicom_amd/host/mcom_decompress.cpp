// minicom_amd/host/mcom_decompress.cpp -- inverse of the stream files written by mcomh_cluster_dump
// (= the reference's cluster_dump at one thread, single-end, not order-preserving).
//
// Restates the reference decoder for that mode (decompress.c: decomp_AATTNN_nonorder :646, decomp_single_nonorder
// :612, decompress_nonorder :495, helpers :40-100) so that losslessness (parity level P2) can be
// proven on a machine where the reference does not exist.  Plain host code, no GPU.
//
// One walker (walk_streams) rebuilds every read of a folder once, in the order of the stream files; what becomes of a read is the
// sink's business, and the three modes are three sinks: AppendSink (default), OrderSink (-p), PairSink (paired end).  What a folder of
// each mode holds is stated in mcom_streams.hpp, which the GPU decoder reads too.
#include "../../include/mcom_host.h"
#include "mcom_ragged.hpp"
#include "mcom_agree.hpp"
#include "mcom_range.hpp"
#include "mcom_streams.hpp"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace mcom_streams;

namespace {

struct DnaReader {                      // getDNAcode (decompress.c:56-74): 4 bases per byte, low bits first
	const std::vector<uint8_t> &b; size_t pos = 0; int k = 4; unsigned cur = 0;
	explicit DnaReader(const std::vector<uint8_t> &b_) : b(b_) {}
	int next() { if (k >= 4) { if (pos >= b.size()) return -1; cur = b[pos++]; k = 0; } int c = (int)(cur & 3); cur >>= 2; ++k; return c; }
};
struct BitReader {                      // getDir (decompress.c:40-54): 8 flags per byte, low bit first
	const std::vector<uint8_t> *b = nullptr; size_t pos = 0; int k = 8; unsigned cur = 0;
	BitReader() {}
	explicit BitReader(const std::vector<uint8_t> &b_) : b(&b_) {}
	int next() { if (k >= 8) { cur = pos < b->size() ? (*b)[pos++] : 0; k = 0; } int c = (int)(cur & 1); cur >>= 1; ++k; return c; }
};

// text of a read against a reference string: letters are literal bases, digits a run of matching bases
// (decompress.c:573-590); the missing tail matches
// The archive is untrusted input: a digit run that would read past the L bases of the reference string, a character
// that is neither a base letter nor a digit, or a line that decodes to more than L bases is an error, not a crash.
bool decode_line(const char *txt, size_t n, const char *ref, int L, std::string &seq)
{
	seq.clear();
	long eq = 0;
	for (size_t i = 0; i < n; ++i) {
		const char ch = txt[i];
		if (ch >= 'A' && ch <= 'Z') {
			if ((long)seq.size() + eq + 1 > (long)L) return false;
			for (long j = 0; j < eq; ++j) seq.push_back(ref[seq.size()]);
			eq = 0;
			seq.push_back(ch);
		} else if (ch >= '0' && ch <= '9') {
			eq = eq * 10 + (ch - '0');
			if (eq > (long)L) return false;
		} else return false;
	}
	while ((int)seq.size() < L) seq.push_back(ref[seq.size()]);
	return (int)seq.size() == L;
}

void shut(FILE *f) { if (f) fclose(f); }                      // (the routes that hand their rows out open no file)

void revcomp(std::string &s)
{
	const size_t n = s.size();
	for (size_t i = 0, j = n ? n - 1 : 0; i < j; ++i, --j) std::swap(s[i], s[j]);
	for (char &c : s) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N';
}

// one read per line; no file is left when it cannot be written whole
bool write_rows(const char *path, const char *rows, uint64_t n, int L)
{
	FILE *out = fopen(path, "wb");
	bool ok = out != nullptr;
	for (uint64_t i = 0; i < n && ok; ++i) ok = fwrite(rows + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
	if (out && fclose(out) != 0) ok = false;
	if (!ok) remove(path);
	return ok;
}

// ---- the sinks.  The walker asks a sink for the row of the next read (row) and hands it the read (put: false ends the walk at once); it
// tells the sink which section's (lists) or stream set's (set) companion streams are current, and asks whether the section has reads left (more).
struct SinkBase {
	void lists(const SectionFiles &) {}
	void set(const SetFiles &) {}
	bool more() const { return true; }
};

// default mode: the reads in stream order, written as they come or -- keep -- appended as rows of L characters; the row is the running count
struct AppendSink : SinkBase {
	const int L; std::vector<char> *keep; FILE *out; uint64_t total = 0;
	AppendSink(int L_, const char *path, std::vector<char> *keep_) : L(L_), keep(keep_), out(keep_ ? nullptr : fopen(path, "w")) {}
	~AppendSink() { shut(out); }
	bool ready() const { return keep || out; }
	bool row(bool, uint64_t &r) { r = total; return true; }
	bool put(uint64_t, const std::string &s)
	{
		if ((int)s.size() != L) return false;
		if (keep) keep->insert(keep->end(), s.begin(), s.end()); else { fwrite(s.data(), 1, s.size(), out); fputc('\n', out); }
		++total;
		return true;
	}
	bool finish() { shut(out); out = nullptr; return !keep || keep->size() == (size_t)total * (size_t)L; }
};

// -p (decomp_AATTNN_order, decompress.c:299-493, decomp_single_order :238-297, decompress_order :109-236): the reads are rebuilt into a
// table indexed by their original position.  Id streams are uint32; a list's ids are delta coded (lists are sorted by id); in ids.bin.T a
// member carries its id when it is the first of its contig or starts at a new position, else the difference to the previous member's id
// (:164-167), and the sum is taken modulo 2^32.
struct OrderSink : SinkBase {
	const int L; const uint64_t n;
	std::vector<char> table; std::vector<uint8_t> seen; bool bad = false;
	const std::vector<uint8_t> *ids = nullptr; size_t p = 0; uint64_t pre = 0; bool in_set = false;   // the current id stream
	OrderSink(int L_, uint64_t n_seq) : L(L_), n(n_seq), table((size_t)n_seq * (size_t)L_, 0), seen((size_t)n_seq, 0) {}
	void lists(const SectionFiles &f) { ids = &f.ids; p = 0; pre = 0; in_set = false; }
	void set(const SetFiles &f) { ids = &f.ids; p = 0; pre = 0; in_set = true; }
	bool more() const { return p + 4 <= ids->size(); }
	bool row(bool diff, uint64_t &r)
	{
		if (!more()) return false;
		uint32_t v; memcpy(&v, ids->data() + p, 4); p += 4;
		pre = diff ? pre + v : v;
		r = in_set ? pre & 0xFFFFFFFFull : pre;
		return true;
	}
	bool put(uint64_t idx, const std::string &s)
	{
		if (idx >= n || (int)s.size() != L || seen[idx]) bad = true;
		else { memcpy(table.data() + idx * (size_t)L, s.data(), (size_t)L); seen[idx] = 1; }
		return true;
	}
	bool finish()
	{
		if (bad) return false;
		for (uint8_t s : seen) if (!s) return false;                       // every position filled exactly once
		return true;
	}
};

// paired end (decomp_AATTNN_pe, decompress.c:963-1212, decompress_pe :780-917): reads of the first file go to it in stream order (the eight
// sections, then the contig members), written as they come or -- keep1 -- appended; a read of the second file carries the line number of its
// mate (peids streams, one file bit per read says which kind a read is) and goes to that row of the table: row i of the two is a pair.
struct PairSink : SinkBase {
	const int L; const uint64_t half;
	std::vector<char> table; std::vector<uint8_t> seen; std::vector<char> *keep1; FILE *out; uint64_t left = 0; bool bad = false;
	const SetFiles *f = nullptr; BitReader bits; size_t ip = 0;            // file bits + mate numbers: .sp for the sections, then one pair per stream set
	PairSink(int L_, uint64_t half_, const char *path1, std::vector<char> *keep1_)
		: L(L_), half(half_), table((size_t)half_ * (size_t)L_, 0), seen((size_t)half_, 0), keep1(keep1_), out(keep1_ ? nullptr : fopen(path1, "w")) {}
	~PairSink() { shut(out); }
	bool ready() const { return keep1 || out; }
	void set(const SetFiles &s) { f = &s; bits = BitReader(s.fb); ip = 0; }
	bool row(bool, uint64_t &r) { r = 0; return true; }
	bool put(uint64_t, const std::string &s)
	{
		if ((int)s.size() != L) { bad = true; return true; }
		if (bits.next()) {                                                 // a read of the second file: to its mate's line
			uint32_t v = 0;
			if (ip + 4 > f->pe.size()) { bad = true; return true; }
			memcpy(&v, f->pe.data() + ip, 4); ip += 4;
			if (v >= half || seen[v]) { bad = true; return true; }
			memcpy(table.data() + (size_t)v * L, s.data(), (size_t)L); seen[v] = 1;
		} else { if (keep1) keep1->insert(keep1->end(), s.begin(), s.end()); else { fwrite(s.data(), 1, s.size(), out); fputc('\n', out); } ++left; }
		return true;
	}
	bool finish()
	{
		shut(out); out = nullptr;
		if (bad || left != half) return false;
		for (uint8_t s : seen) if (!s) return false;
		return true;
	}
};

// ---- the walk: every read of a folder once, sections in the order of SECTIONS, then the contig sets; false = the folder is refused.
// agree (DEFAULT and ORDER): the member loop's report to the agreement mask.
template <class Sink> bool walk_streams(Mode mode, const std::string &dir, const StreamInfo &I, Sink &sink, McomAgreeSink *agree = nullptr)
{
	const int L = I.L;
	const long counted[3] = {I.na, I.nt, I.nn};
	std::string seq;
	uint64_t row = 0;
	auto give = [&](const std::string &s) { return sink.row(true, row) && sink.put(row, s); };   // a section's read: a short id stream refuses the folder
	SetFiles sp;
	if (mode == PE) { if (!load_pairing(dir, ".sp", sp)) return false; sink.set(sp); }
	for (int s = 0; s < N_SECTIONS; ++s) {
		const Section &S = SECTIONS[s];
		SectionFiles f;
		if (!load_section(mode, dir, s, f)) return false;
		sink.lists(f);
		const char *txt = (const char*)f.data.data();
		if (S.kind == COUNTED) {                                           // all-A / all-T / all-N reads are only counted (decompress.c:660-688, -p :320-372)
			for (long i = 0; i < counted[s]; ++i) if (!give(std::string((size_t)L, S.base))) return false;
		} else if (S.kind == PACKED) {                                     // unclustered reads, 2 bits per base (:612-644, -p :238-280)
			// floor(4 bytes / L) reads: a trailing partial read is padding; -p stops quietly where singleFile.ids.bin ends, because
			// padding of the last byte can look like one more read of A
			const size_t whole = f.data.size() * 4 / (size_t)L;
			DnaReader r(f.data);
			for (size_t i = 0; i < whole && sink.more(); ++i) {
				seq.clear();
				for (int j = 0; j < L; ++j) seq.push_back("ACGT"[r.next() & 3]);
				if (!give(seq)) return false;
			}
		} else {                                                           // near-constant reads: text against a constant base (:690-760, -p :374-493); reads kept as text because they contain N (-p :282-296)
			const std::string cref((size_t)L, S.base);
			size_t b = 0;
			for (size_t i = 0; i < f.data.size(); ++i) if (txt[i] == '\n') {
				// a kept line whose length is not L refuses the folder in put(): at once where reads are appended, at the end where they are placed
				if (S.kind == VERBATIM) seq.assign(txt + b, i - b); else if (!decode_line(txt + b, i - b, cref.c_str(), L, seq)) return false;
				b = i + 1;
				if (!give(seq)) return false;
			}
		}
	}
	// contigs and their reads, one stream set per writer thread (:495-610, -p :109-236, paired end :780-917)
	for (int th = 0; th < I.nth; ++th) {
		SetFiles f;
		if (!load_set(mode, dir, th, f)) return false;
		sink.set(f);
		DnaReader rr(f.ref); BitReader dr(f.dir);
		size_t pp = 0, dp = 0;
		std::string ref;
		uint64_t coff = 0;                                                  // bases of ref.bin before this contig (the agreement mask's places)
		if (agree) agree->L = L;
		while (pp + 4 <= f.pos.size()) {
			uint32_t num; memcpy(&num, f.pos.data() + pp, 4); pp += 4;
			ref.clear();
			int pre = 0;
			for (uint32_t q = 0; q < num; ++q) {
				if (pp + 2 > f.pos.size()) return false;
				uint16_t d; memcpy(&d, f.pos.data() + pp, 2); pp += 2;
				if (!sink.row(q > 0 && d == 0, row)) return false;         // -p: same begin position: the id is a difference (:178-181)
				const int pos = pre + d; pre = pos;
				while ((int)ref.size() < pos + L) { const int c = rr.next(); if (c < 0) return false; ref.push_back("ACGT"[c]); }   // getRef (:92-100)
				const int rev = dr.next();
				size_t e = dp; while (e < f.dif.size() && f.dif[e] != '\n') ++e;
				if (e >= f.dif.size() || !decode_line((const char*)f.dif.data() + dp, e - dp, ref.c_str() + pos, L, seq)) return false;
				dp = e + 1;
				if (agree) agree->member(row, coff + (uint64_t)pos, rev, seq.data(), ref.c_str() + pos);
				if (rev) revcomp(seq);
				if (!sink.put(row, seq)) return false;
			}
			coff += ref.size();
		}
		if (agree) agree->end_set();
	}
	return true;
}

// info.txt and the first size checks: nothing is allocated or opened for a folder that fails them
bool open_folder(Mode mode, const char *folder, StreamInfo &I) { return read_info(mode, folder, I) && counts_fit(mode, folder, I); }

// no C++ exception crosses the C boundary (a corrupt info.txt can ask for more memory than there is)
template <class F> int guard(F f) { try { return f(); } catch (...) { return -1; } }

} // namespace

// keep: the rows (L characters each, back to back) are handed out instead of being written (mcomh_decompress_fastq_reordered)
static int decompress_impl(const char *folder, const char *out_path, uint64_t *n_reads, std::vector<char> *keep = nullptr, int *L_out = nullptr, McomAgreeSink *agree = nullptr)
{
	StreamInfo I;
	if (!folder || (!out_path && !keep) || !open_folder(DEFAULT, folder, I)) return -1;
	AppendSink sink(I.L, out_path, keep);
	if (!sink.ready() || !walk_streams(DEFAULT, folder, I, sink, agree) || !sink.finish()) return -1;
	if (L_out) *L_out = I.L;
	if (n_reads) *n_reads = sink.total;
	return 0;
}

// ---- order-preserving mode (-p): the table is written out in the original order once every position has been filled exactly once
// keep: the table of n_seq x L characters is handed out instead of being written (mcomh_decompress_fastq)
static int decompress_order_impl(const char *folder, const char *out_path, uint64_t *n_reads, std::vector<char> *keep = nullptr, int *L_out = nullptr, McomAgreeSink *agree = nullptr)
{
	StreamInfo I;
	if (!folder || (!out_path && !keep) || !open_folder(ORDER, folder, I)) return -1;
	OrderSink sink(I.L, I.n_seq);
	if (!walk_streams(ORDER, folder, I, sink, agree) || !sink.finish()) return -1;
	if (keep) keep->swap(sink.table); else if (!write_rows(out_path, sink.table.data(), I.n_seq, I.L)) return -1;
	if (L_out) *L_out = I.L;
	if (n_reads) *n_reads = I.n_seq;
	return 0;
}

// ---- paired end (_PE): line i of the two outputs is a pair
// keep1 / keep2: the rows of the two files (L characters each) are handed out instead of being written (mcomh_decompress_fastq_pe)
static int decompress_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, std::vector<char> *keep1 = nullptr, std::vector<char> *keep2 = nullptr,
                              int *L_out = nullptr)
{
	const bool keep = keep1 && keep2;
	StreamInfo I;
	if (!folder || (!keep && (!out_path1 || !out_path2)) || !open_folder(PE, folder, I)) return -1;
	PairSink sink(I.L, (uint64_t)I.half, out_path1, keep ? keep1 : nullptr);
	if (!sink.ready() || !walk_streams(PE, folder, I, sink) || !sink.finish()) return -1;
	if (keep) keep2->swap(sink.table); else if (!write_rows(out_path2, sink.table.data(), (uint64_t)I.half, I.L)) return -1;
	if (L_out) *L_out = I.L;
	if (n_pairs) *n_pairs = (uint64_t)I.half;
	return 0;
}

extern "C" int mcomh_decompress(const char *folder, const char *out_path, uint64_t *n_reads)
{
	return guard([&] { return decompress_impl(folder, out_path, n_reads); });
}

// ---- the side members of an archive, and the FASTQ records made of them -----------------------------------------------------------------
namespace {
// the rows [first, first + count) of a quality member (mcomh_qual_decode_rows: the touched segments alone, no CRC of the whole)
struct Range { uint64_t first, count; };

// a `.mcq` member that must state n rows of L bytes: all of its rows, or those of rng, at pitch L
bool decode_quals(const std::vector<uint8_t> &member, uint64_t n, int L, std::vector<uint8_t> &quals, const Range *rng = nullptr)
{
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcomh_qual_info(member.data(), member.size(), &qn, &qL) || qn != n || (int)qL != L) return false;
	quals.assign((size_t)(rng ? rng->count : n) * (size_t)L + 1, 0);
	const int rc = rng ? mcomh_qual_decode_rows(member.data(), member.size(), rng->first, rng->count, quals.data(), (uint64_t)L, &qn, &qL)
	                   : mcomh_qual_decode(member.data(), member.size(), quals.data(), (uint64_t)L, n, &qn, &qL);
	return !rc && qn == n && (int)qL == L;
}
bool load_quals(const std::string &path, uint64_t n, int L, std::vector<uint8_t> &quals, const Range *rng = nullptr)
{
	std::vector<uint8_t> member;
	return slurp(path, member) && decode_quals(member, n, L, quals, rng);
}

// a decoded name text: two lines per record (the name, the '+' text), `at` the start of every line and the text's end
struct NameText { std::vector<uint8_t> text; std::vector<uint64_t> at; uint64_t len = 0; };

// a `.mcn` member that must state n records; mate: a member of kind 2, coded against the decoded text of the first file's names
bool decode_names(const std::vector<uint8_t> &member, uint64_t n, NameText &t, const NameText *mate = nullptr)
{
	uint64_t nn = 0, tl = 0;
	if ((mate ? mcomh_name_info_mate(member.data(), member.size(), &nn, &tl) : mcomh_name_info(member.data(), member.size(), &nn, &tl)) || nn != n) return false;
	t.text.resize(tl + 1);
	if ((mate ? mcomh_name_decode_mate(member.data(), member.size(), mate->text.data(), mate->len, t.text.data(), tl, &tl, &nn)
	          : mcomh_name_decode(member.data(), member.size(), t.text.data(), tl, &tl, &nn)) || nn != n) return false;
	t.len = tl;
	t.at.clear(); t.at.reserve(2 * n + 1); t.at.push_back(0);
	for (uint64_t i = 0; i < t.len; ++i) if (t.text[i] == '\n') t.at.push_back(i + 1);
	return t.at.size() == 2 * n + 1;
}

// dir/name (`minicom -N`): named = the archive has it; false: it has it, and it is refused or of another number
bool load_names(const std::string &dir, const char *name, uint64_t n, NameText &t, bool &named)
{
	std::vector<uint8_t> member;
	named = slurp(dir + "/" + name, member);
	return !named || decode_names(member, n, t);
}

// name_1.mcn (kind 0 or 1) and name_2.mcn, which is decoded with the decoded name_1 text as its mate (section 3.12)
bool load_pair_names(const std::string &dir, uint64_t n, NameText nm[2], bool &named)
{
	std::vector<uint8_t> m1, m2;
	named = slurp(dir + "/name_1.mcn", m1);
	if (named != slurp(dir + "/name_2.mcn", m2)) return false;            // name_2 is coded against name_1; one alone is no archive
	return !named || (decode_names(m1, n, nm[0]) && decode_names(m2, n, nm[1], &nm[0]));
}

// reads, quals: rows of L characters, row 0 the first record written; names NULL: records `@<i+1>` with a bare '+'.  base: the number the
// first record has in the archive (a range, section 3.19): it picks the names and numbers the records
bool write_records_named(const char *path, const char *reads, const std::vector<uint8_t> &quals, const NameText *names, uint64_t n, int L, uint64_t base = 0)
{
	FILE *out = fopen(path, "wb");
	if (!out) return false;
	bool ok = true;
	for (uint64_t i = 0; i < n && ok; ++i) {
		if (names) {
			const uint64_t a = names->at[2 * (base + i)], b = names->at[2 * (base + i) + 1], c = names->at[2 * (base + i) + 2];
			ok = fputc('@', out) != EOF && fwrite(names->text.data() + a, 1, b - a, out) == b - a && fwrite(reads + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputs("\n+", out) >= 0 &&
			     fwrite(names->text.data() + b, 1, c - b, out) == c - b;
		} else
			ok = fprintf(out, "@%llu\n", (unsigned long long)(base + i + 1)) > 0 && fwrite(reads + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputs("\n+\n", out) >= 0;
		ok = ok && fwrite(quals.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
	}
	if (fclose(out) != 0 || !ok) { remove(path); return false; }
	return true;
}
}  // namespace

// ---- a ragged archive (`minicom -p -V`): folder/len.bin says which records are the core's reads of L bases and
// which lie in odd.seq / odd.qual.  The core's reads (and qual.mcq's rows) are decoded as ever, then the records are laid out in input
// order by mcomh_fastq_emit_ragged: one read per line, or -- fastq -- four-line records named by name.mcn or `@<i+1>`.  A folder whose
// parts disagree is refused and no file is written.
static int decompress_ragged_impl(const char *folder, const char *out_path, uint64_t *n_reads, bool fastq)
{
	if (!folder || !out_path) return -1;
	const std::string dir(folder);
	std::vector<char> reads; int L = 0; uint64_t n_even = 0;
	if (decompress_order_impl(folder, nullptr, &n_even, &reads, &L)) return -1;
	std::vector<uint8_t> qmember, nmember, quals;
	const bool has_qual = slurp(dir + "/qual.mcq", qmember), named = slurp(dir + "/name.mcn", nmember);
	if (fastq && !has_qual) return -1;
	McomRaggedParts P;
	std::string why;
	if (!mcom_ragged_load(folder, L, n_even, has_qual, P, why)) { fprintf(stderr, "minicom decoder: %s\n", why.c_str()); return -1; }
	uint64_t qn = 0, nn = 0, tl = 0; uint32_t qL = 0;
	if (has_qual && (mcomh_qual_info(qmember.data(), qmember.size(), &qn, &qL) || qn != n_even || (int)qL != L)) { fprintf(stderr, "minicom decoder: qual.mcq does not state the number and length of the reads of the modal length\n"); return -1; }
	if (named && (mcomh_name_info(nmember.data(), nmember.size(), &nn, &tl) || nn != P.n)) { fprintf(stderr, "minicom decoder: name.mcn does not state the records' number\n"); return -1; }
	mcomh_ragged_src S;
	memset(&S, 0, sizeof S);
	S.reads = (const uint8_t*)reads.data(); S.read_pitch = (uint64_t)L; S.n_even = n_even; S.L = (uint32_t)L;
	S.odd_seq = P.odd_seq.data(); S.odd_bytes = P.odd_seq.size(); S.slot = P.slot.data(); S.len = P.len.data(); S.n = P.n;
	NameText names;
	std::vector<uint64_t> rec_off;
	if (fastq) {
		if (!decode_quals(qmember, n_even, L, quals)) return -1;
		S.quals = quals.data(); S.qual_pitch = (uint64_t)L; S.odd_qual = P.odd_qual.data();
		if (named) {
			if (!decode_names(nmember, P.n, names)) return -1;
			for (uint64_t i = 0; i <= P.n; ++i) rec_off.push_back(names.at[2 * i]);   // the records' offsets: every second line
			S.names = names.text.data(); S.names_bytes = names.len; S.rec_off = rec_off.data();
		}
	}
	uint64_t bytes = 0;
	if (mcomh_fastq_emit_ragged(&S, 0, P.n, nullptr, 0, &bytes)) { fprintf(stderr, "minicom decoder: the parts of the ragged archive disagree\n"); return -1; }
	std::vector<uint8_t> out((size_t)bytes + 1);
	if (mcomh_fastq_emit_ragged(&S, 0, P.n, out.data(), bytes, &bytes)) return -1;
	FILE *f = fopen(out_path, "wb");
	if (!f) return -1;
	const bool ok = !bytes || fwrite(out.data(), 1, (size_t)bytes, f) == bytes;
	if (fclose(f) != 0 || !ok) { remove(out_path); return -1; }
	if (n_reads) *n_reads = P.n;
	return 0;
}

extern "C" int mcomh_decompress_order(const char *folder, const char *out_path, uint64_t *n_reads)
{
	return guard([&] { return folder && mcom_ragged_present(folder) ? decompress_ragged_impl(folder, out_path, n_reads, false) : decompress_order_impl(folder, out_path, n_reads); });
}

extern "C" int mcomh_decompress_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	return guard([&] { return decompress_pe_impl(folder, out_path1, out_path2, n_pairs); });
}

// ---- a -p -Q archive back to FASTQ on the host: the reads of decompress_order_impl in memory, the quality
// rows of folder/qual.mcq by the host twin, then records `@<i+1>`, read, `+`, qualities.  The cross-check of mcomh_decompress_fastq_gpu:
// the same bytes, the same archives refused (one that is not a -p archive, no qual.mcq, another n or L than the reads).  With
// folder/name.mcn (section 3.10) the records are `@<name>`, read, `+<text>`, qualities; a name.mcn of another n or a refused one is an error.
static int decompress_fastq_impl(const char *folder, const char *out_path, uint64_t *n_reads)
{
	if (!folder || !out_path) return -1;
	const std::string dir(folder);
	std::vector<char> reads; int L = 0; uint64_t n = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L)) return -1;
	std::vector<uint8_t> quals; NameText names; bool named = false;
	if (!load_quals(dir + "/qual.mcq", n, L, quals) || !load_names(dir, "name.mcn", n, names, named)) return -1;
	if (!write_records_named(out_path, reads.data(), quals, named ? &names : nullptr, n, L)) return -1;
	if (n_reads) *n_reads = n;
	return 0;
}

extern "C" int mcomh_decompress_fastq(const char *folder, const char *out_path, uint64_t *n_reads)
{
	return guard([&] { return folder && mcom_ragged_present(folder) ? decompress_ragged_impl(folder, out_path, n_reads, true) : decompress_fastq_impl(folder, out_path, n_reads); });
}

// ---- `minicom -q` archives back to FASTQ on the host: the rows of the default / paired-end decoder in memory,
// the quality rows of folder/rqual.mcq (paired end: rqual_1.mcq and rqual_2.mcq) by the host twin -- they are stored in the archive's
// own order, row j beside read j -- then records `@<j+1>`, read, `+`, qualities.  The cross-check of the _gpu routes: the same bytes,
// the same archives refused (-p archives, an archive of the other kind, a missing member, one of another n or L than the reads, a
// refused member); no output file is left then.
static int decompress_fastq_reordered_impl(const char *folder, const char *out_path, uint64_t *n_reads)
{
	if (!folder || !out_path) return -1;
	const std::string dir(folder);
	if (exists(dir + "/allA.ids.bin") || exists(dir + "/file.bin.sp")) return -1;      // a -p or a paired-end archive
	std::vector<char> reads; int L = 0; uint64_t n = 0;
	if (decompress_impl(folder, nullptr, &n, &reads, &L)) return -1;
	std::vector<uint8_t> quals;
	if (!load_quals(dir + "/rqual.mcq", n, L, quals) || !write_records_named(out_path, reads.data(), quals, nullptr, n, L)) return -1;
	if (n_reads) *n_reads = n;
	return 0;
}

// two files of n records each; neither is left when the second cannot be written
static bool write_record_pair(const char *out_path1, const char *out_path2, const char *r1, const char *r2, const std::vector<uint8_t> q[2], const NameText *nm, uint64_t n, int L, uint64_t base = 0)
{
	if (!write_records_named(out_path1, r1, q[0], nm ? &nm[0] : nullptr, n, L, base)) return false;
	if (!write_records_named(out_path2, r2, q[1], nm ? &nm[1] : nullptr, n, L, base)) { remove(out_path1); return false; }
	return true;
}

static int decompress_fastq_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	const std::string dir(folder);
	if (exists(dir + "/allA.ids.bin")) return -1;                                       // a -p archive
	std::vector<char> r1, r2; int L = 0; uint64_t n = 0;
	if (decompress_pe_impl(folder, nullptr, nullptr, &n, &r1, &r2, &L)) return -1;
	std::vector<uint8_t> q[2];
	if (!load_quals(dir + "/rqual_1.mcq", n, L, q[0]) || !load_quals(dir + "/rqual_2.mcq", n, L, q[1])) return -1;
	if (!write_record_pair(out_path1, out_path2, r1.data(), r2.data(), q, nullptr, n, L)) return -1;
	if (n_pairs) *n_pairs = n;
	return 0;
}

extern "C" int mcomh_decompress_fastq_reordered(const char *folder, const char *out_path, uint64_t *n_reads)
{
	return guard([&] { return decompress_fastq_reordered_impl(folder, out_path, n_reads); });
}

extern "C" int mcomh_decompress_fastq_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	return guard([&] { return decompress_fastq_pe_impl(folder, out_path1, out_path2, n_pairs); });
}

// ---- a pair kept in input order (`minicom -1 -2 -p [-Q [-N]]`) on the host: the 2 n rows of decompress_order_impl,
// rows [0, n) to the first file and [n, 2 n) to the second.  folder/pe_order.txt (one line, n) must agree with the reads' number.  With
// quality values: qual_1.mcq and qual_2.mcq, n rows each; with names: name_1.mcn and name_2.mcn.  The cross-check of the _gpu routes: the
// same bytes, the same archives refused; neither file is left.
static int decompress_order_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	std::vector<char> reads; int L = 0; uint64_t n = 0, half = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L) || !pair_count(folder, n, half)) return -1;
	if (!write_rows(out_path1, reads.data(), half, L)) return -1;
	if (!write_rows(out_path2, reads.data() + half * (size_t)L, half, L)) { remove(out_path1); return -1; }
	if (n_pairs) *n_pairs = half;
	return 0;
}

static int decompress_fastq_order_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	const std::string dir(folder);
	std::vector<char> reads; int L = 0; uint64_t n = 0, half = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L) || !pair_count(dir, n, half)) return -1;
	std::vector<uint8_t> q[2]; NameText nm[2]; bool named = false;
	if (!load_quals(dir + "/qual_1.mcq", half, L, q[0]) || !load_quals(dir + "/qual_2.mcq", half, L, q[1]) || !load_pair_names(dir, half, nm, named)) return -1;
	if (!write_record_pair(out_path1, out_path2, reads.data(), reads.data() + half * (size_t)L, q, named ? nm : nullptr, half, L)) return -1;
	if (n_pairs) *n_pairs = half;
	return 0;
}

extern "C" int mcomh_decompress_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	return guard([&] { return decompress_order_pe_impl(folder, out_path1, out_path2, n_pairs); });
}

extern "C" int mcomh_decompress_fastq_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	return guard([&] { return decompress_fastq_order_pe_impl(folder, out_path1, out_path2, n_pairs); });
}

// ---- a record range of a -p archive (`minicom -d -R FIRST:COUNT`) -------------------------------------------
// The host route is the specification and the cross-check, not a fast path: the whole table by decompress_order_impl -- so every check of
// the full decode is made -- then the slice.  Quality rows come from mcomh_qual_decode_rows, which decodes the touched segments alone
// and, like the device, cannot check the member's CRC for a part; the names are decoded whole.  The refusals that need no decoding are
// made here for both routes, before a file is written.
namespace {
const char *range_refusal(const std::string &dir)
{
	if (!exists(dir + "/info.txt")) return "no info.txt: not a folder of stream files";
	if (exists(dir + "/rqual.mcq") || exists(dir + "/rqual_1.mcq") || exists(dir + "/rqual_2.mcq")) return "an archive made with -q keeps its records in an order of its own: there is no input order to count a range in";
	if (!exists(dir + "/allA.ids.bin")) return "not a -p archive: there is no input order to count a range in";
	if (mcom_ragged_present(dir.c_str())) return "an archive made with -V (len.bin): a range of records of differing lengths is not built";
	return nullptr;
}

int range_host(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, bool pair, bool fastq)
{
	const std::string dir(folder);
	std::vector<char> reads; int L = 0; uint64_t n_rows = 0, n = 0;
	if (decompress_order_impl(folder, nullptr, &n_rows, &reads, &L)) { fprintf(stderr, "minicom decoder: %s is not a complete, consistent -p archive\n", folder); return -1; }
	n = n_rows;
	if (pair && !pair_count(dir, n_rows, n)) { fprintf(stderr, "minicom decoder: %s: no pe_order.txt that states half the reads' number: not a pair kept in input order\n", folder); return -1; }
	if (first > n) { fprintf(stderr, "minicom decoder: the range begins at record %llu (from 0), the archive holds %llu\n", (unsigned long long)first, (unsigned long long)n); return -1; }
	if (count > n - first) count = n - first;
	const char *rows1 = reads.data() + first * (size_t)L, *rows2 = rows1 + n * (size_t)L;   // (rows2: a pair's second file)
	if (fastq) {
		const Range rng{first, count};
		const char *qname[2] = {pair ? "/qual_1.mcq" : "/qual.mcq", "/qual_2.mcq"};
		std::vector<uint8_t> q[2]; NameText nm[2]; bool named = false;
		for (int k = 0; k < (pair ? 2 : 1); ++k) if (!load_quals(dir + qname[k], n, L, q[k], &rng)) { fprintf(stderr, "minicom decoder: %s%s is missing, refused or states another number or length than the reads\n", folder, qname[k]); return -1; }
		if (!(pair ? load_pair_names(dir, n, nm, named) : load_names(dir, "name.mcn", n, nm[0], named))) return -1;
		if (!(pair ? write_record_pair(out_path1, out_path2, rows1, rows2, q, named ? nm : nullptr, count, L, first)
		           : write_records_named(out_path1, rows1, q[0], named ? &nm[0] : nullptr, count, L, first))) return -1;
	} else {
		if (!write_rows(out_path1, rows1, count, L)) return -1;
		if (pair && !write_rows(out_path2, rows2, count, L)) { remove(out_path1); return -1; }
	}
	if (n_written) *n_written = count;
	return 0;
}

int range_any(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, int device, bool pair, bool fastq)
{
	if (!folder || !out_path1 || (pair && !out_path2)) return -1;
	if (const char *why = range_refusal(folder)) { fprintf(stderr, "minicom decoder: a range of %s is refused: %s\n", folder, why); return -1; }
	return guard([&] {
		if (device < 0) return range_host(folder, out_path1, out_path2, first, count, n_written, pair, fastq);
#ifdef MCOM_ENTROPY_HOST_ONLY
		fprintf(stderr, "minicom decoder: this build has no GPU route\n");
		return -1;
#else
		return mcom_range_gpu(folder, out_path1, out_path2, first, count, n_written, device, pair, fastq);
#endif
	});
}
}  // namespace

extern "C" int mcomh_decompress_order_range(const char *folder, const char *out_path, uint64_t first, uint64_t count, uint64_t *n_written, int device)
{
	return range_any(folder, out_path, nullptr, first, count, n_written, device, false, false);
}
extern "C" int mcomh_decompress_fastq_range(const char *folder, const char *out_path, uint64_t first, uint64_t count, uint64_t *n_written, int device)
{
	return range_any(folder, out_path, nullptr, first, count, n_written, device, false, true);
}
extern "C" int mcomh_decompress_order_pe_range(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, int device, int fastq)
{
	return range_any(folder, out_path1, out_path2, first, count, n_written, device, true, fastq != 0);
}

// ---- the agreement mask of a folder on the host (`minicom -a Q[:C]`): the default / -p decoder with its rows kept
// in memory -- the same validations, the same refusals -- and the member loop's report to a McomAgreeSink.  The twin of mcom_agree_mask_gpu.
int mcom_agree_mask_host(const char *folder, bool order, int C, std::vector<uint8_t> &mask, uint64_t *n_rows, int *L_out)
{
	if (!folder || C < 1 || C > 255) return -1;
	return guard([&] {
		McomAgreeSink sink; sink.C = C;
		std::vector<char> reads; int L = 0; uint64_t n = 0;
		if (order ? decompress_order_impl(folder, nullptr, &n, &reads, &L, &sink) : decompress_impl(folder, nullptr, &n, &reads, &L, &sink)) return -1;
		const size_t mb = (size_t)(L + 7) / 8;
		mask.assign((size_t)n * mb, 0);
		for (const McomAgreeSink::Row &r : sink.rows) { if (r.row >= n) return -1; memcpy(mask.data() + (size_t)r.row * mb, r.bits, mb); }
		if (n_rows) *n_rows = n;
		if (L_out) *L_out = L;
		return 0;
	});
}
