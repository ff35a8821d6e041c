// minicom_amd/host/mcom_decompress.cpp -- inverse of the stream files written by mcomh_cluster_dump
// (= the reference's cluster_dump at one thread, single-end, not order-preserving).
//
// Restates the reference decoder for that mode (decompress.c: decomp_AATTNN_nonorder :646, decomp_single_nonorder
// :612, decompress_nonorder :495, helpers :40-100) so that losslessness (parity level P2) can be
// proven on a machine where the reference does not exist.  Plain host code, no GPU.
#include "../../include/mcom_host.h"
#include "mcom_ragged.hpp"
#include "mcom_agree.hpp"
#include "mcom_range.hpp"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
	out.resize((size_t)n);
	size_t got = n ? fread(out.data(), 1, (size_t)n, f) : 0;
	fclose(f);
	return got == (size_t)n;
}

struct DnaReader {                      // getDNAcode (decompress.c:56-74): 4 bases per byte, low bits first
	const std::vector<uint8_t> &b; size_t pos = 0; int k = 4; unsigned cur = 0;
	explicit DnaReader(const std::vector<uint8_t> &b_) : b(b_) {}
	int next() { if (k >= 4) { if (pos >= b.size()) return -1; cur = b[pos++]; k = 0; } int c = (int)(cur & 3); cur >>= 2; ++k; return c; }
};
struct BitReader {                      // getDir (decompress.c:40-54): 8 flags per byte, low bit first
	const std::vector<uint8_t> &b; size_t pos = 0; int k = 8; unsigned cur = 0;
	explicit BitReader(const std::vector<uint8_t> &b_) : b(b_) {}
	int next() { if (k >= 8) { cur = pos < b.size() ? b[pos++] : 0; k = 0; } int c = (int)(cur & 1); cur >>= 1; ++k; return c; }
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

size_t file_bytes(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return 0;
	fseek(f, 0, SEEK_END); const long n = ftell(f); fclose(f);
	return n > 0 ? (size_t)n : 0;
}

void shut(FILE *f) { if (f) fclose(f); }                      // (the routes that hand their rows out open no file)

void revcomp(std::string &s)
{
	const size_t n = s.size();
	for (size_t i = 0, j = n ? n - 1 : 0; i < j; ++i, --j) std::swap(s[i], s[j]);
	for (char &c : s) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'N';
}

} // namespace

// keep: the rows (L characters each, back to back) are handed out instead of being written (mcomh_decompress_fastq_reordered)
static int decompress_impl(const char *folder, const char *out_path, uint64_t *n_reads, std::vector<char> *keep = nullptr, int *L_out = nullptr, McomAgreeSink *agree = nullptr)
{
	if (!folder || (!out_path && !keep)) return -1;
	const std::string dir(folder);
	FILE *fi = fopen((dir + "/info.txt").c_str(), "r");
	if (!fi) return -1;
	int L = 0, nth = 0; long na = 0, nt = 0, nn = 0;
	if (fscanf(fi, "%d %d %ld %ld %ld", &L, &nth, &na, &nt, &nn) != 5) { fclose(fi); return -1; }
	fclose(fi);
	if (L < 1 || L > 256 || nth < 1 || nth > 4096 || na < 0 || nt < 0 || nn < 0) return -1;
	FILE *out = keep ? nullptr : fopen(out_path, "w");
	if (!keep && !out) return -1;
	uint64_t total = 0;
	auto line = [&](const std::string &s) { if (keep) { if ((int)s.size() == L) keep->insert(keep->end(), s.begin(), s.end()); } else { fwrite(s.data(), 1, s.size(), out); fputc('\n', out); } ++total; };
	// all-A / all-T / all-N reads are only counted (decompress.c:660-688)
	for (long i = 0; i < na; ++i) line(std::string((size_t)L, 'A'));
	for (long i = 0; i < nt; ++i) line(std::string((size_t)L, 'T'));
	for (long i = 0; i < nn; ++i) line(std::string((size_t)L, 'N'));
	// near-constant reads: text against a constant base (:690-760)
	std::vector<uint8_t> buf;
	std::string seq;
	const char bases[3] = {'A', 'T', 'N'}; const char *names[3] = {"AA.txt", "TT.txt", "NN.txt"};
	for (int q = 0; q < 3; ++q) {
		if (!slurp(dir + "/" + names[q], buf)) { shut(out); return -1; }
		const std::string cref((size_t)L, bases[q]);
		size_t s = 0;
		for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') { if (!decode_line((const char*)buf.data() + s, i - s, cref.c_str(), L, seq)) { shut(out); return -1; } line(seq); s = i + 1; }
	}
	// reads kept as text because they contain N
	if (!slurp(dir + "/single_N.seq", buf)) { shut(out); return -1; }
	{ size_t s = 0; for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') { if (i - s != (size_t)L) { shut(out); return -1; } line(std::string((const char*)buf.data() + s, i - s)); s = i + 1; } }
	// unclustered reads, 2 bits per base (:612-644); a trailing partial byte carries no complete read
	if (!slurp(dir + "/single.seq", buf)) { shut(out); return -1; }
	{
		DnaReader r(buf);
		for (;;) {
			seq.clear();
			int c = 0;
			for (int i = 0; i < L; ++i) { c = r.next(); if (c < 0) break; seq.push_back("ACGT"[c]); }
			if (c < 0 || (int)seq.size() < L) break;
			line(seq);
		}
	}
	// contigs and their reads, one stream set per writer thread (:495-610)
	for (int th = 0; th < nth; ++th) {
		std::vector<uint8_t> bref, bpos, bdir, bdif;
		const std::string sfx = "." + std::to_string(th);
		if (!slurp(dir + "/ref.bin" + sfx, bref) || !slurp(dir + "/beg_pos.bin" + sfx, bpos) || !slurp(dir + "/dir.bin" + sfx, bdir) ||
		    !slurp(dir + "/dif_char.txt" + sfx, bdif)) { shut(out); return -1; }
		DnaReader rr(bref); BitReader dr(bdir);
		size_t pp = 0, dp = 0;
		std::string ref;
		uint64_t coff = 0;                                                  // bases of ref.bin before this contig (the agreement mask's places)
		if (agree) agree->L = L;
		while (pp + 4 <= bpos.size()) {
			uint32_t num; memcpy(&num, bpos.data() + pp, 4); pp += 4;
			ref.clear();
			int pre = 0;
			for (uint32_t q = 0; q < num; ++q) {
				if (pp + 2 > bpos.size()) { shut(out); return -1; }
				uint16_t d; memcpy(&d, bpos.data() + pp, 2); pp += 2;
				const int pos = pre + d; pre = pos;
				while ((int)ref.size() < pos + L) { const int c = rr.next(); if (c < 0) { shut(out); return -1; } ref.push_back("ACGT"[c]); }   // getRef (:92-100)
				const int rev = dr.next();
				size_t e = dp; while (e < bdif.size() && bdif[e] != '\n') ++e;
				if (e >= bdif.size() || !decode_line((const char*)bdif.data() + dp, e - dp, ref.c_str() + pos, L, seq)) { shut(out); return -1; }
				dp = e + 1;
				if (agree) agree->member(total, coff + (uint64_t)pos, rev, seq.data(), ref.c_str() + pos);
				if (rev) revcomp(seq);
				line(seq);
			}
			coff += ref.size();
		}
		if (agree) agree->end_set();
	}
	shut(out);
	if (keep && keep->size() != (size_t)total * (size_t)L) return -1;
	if (L_out) *L_out = L;
	if (n_reads) *n_reads = total;
	return 0;
}

// ---- order-preserving mode (-p): every stream has a companion stream of read ids ------------------------------------
// Restates decomp_AATTNN_order (decompress.c:299-493), decomp_single_order (:238-297) and decompress_order (:109-236):
// the reads are rebuilt into a table indexed by their original position and written out in that order.  Id streams
// are uint32, delta coded inside a list (lists are sorted by id); in ids.bin.T a member carries its id when it is the
// first of its contig or starts at a new position, else the difference to the previous member's id (:164-167).
// keep: the table of n_seq x L characters is handed out instead of being written (mcomh_decompress_fastq)
static int decompress_order_impl(const char *folder, const char *out_path, uint64_t *n_reads, std::vector<char> *keep = nullptr, int *L_out = nullptr, McomAgreeSink *agree = nullptr)
{
	if (!folder || (!out_path && !keep)) return -1;
	const std::string dir(folder);
	FILE *fi = fopen((dir + "/info.txt").c_str(), "r");
	if (!fi) return -1;
	int L = 0, nth = 0; long na = 0, nt = 0, nn = 0; unsigned long n_seq = 0;
	if (fscanf(fi, "%d %d %ld %ld %ld %lu", &L, &nth, &na, &nt, &nn, &n_seq) != 6) { fclose(fi); return -1; }
	fclose(fi);
	if (L < 1 || L > 256 || nth < 1 || nth > 4096 || na < 0 || nt < 0 || nn < 0) return -1;
	{   // every read of this mode has a 4-byte entry in one of the id streams: n_seq cannot exceed what they hold
		size_t idb = 0;
		for (const char *nm : {"allA.ids.bin", "allT.ids.bin", "allN.ids.bin", "AA.ids.bin", "TT.ids.bin", "NN.ids.bin", "singleFile.ids.bin", "Nfile.ids.bin"}) idb += file_bytes(dir + "/" + nm);
		for (int th = 0; th < nth; ++th) idb += file_bytes(dir + "/ids.bin." + std::to_string(th));
		if ((size_t)n_seq > idb / 4) return -1;
	}
	std::vector<char> table((size_t)n_seq * (size_t)L, 0);
	std::vector<uint8_t> seen((size_t)n_seq, 0);
	bool bad = false;
	auto put = [&](uint64_t idx, const std::string &s) {
		if (idx >= n_seq || (int)s.size() != L || seen[idx]) { bad = true; return; }
		memcpy(table.data() + idx * (size_t)L, s.data(), (size_t)L); seen[idx] = 1;
	};
	struct Ids {                                                        // one delta-coded id list
		std::vector<uint8_t> b; size_t p = 0; uint64_t pre = 0;
		bool next(uint64_t &idx) { if (p + 4 > b.size()) return false; uint32_t v; memcpy(&v, b.data() + p, 4); p += 4; pre += v; idx = pre; return true; }
	};
	std::vector<uint8_t> buf;
	std::string seq;
	uint64_t idx = 0;
	// all-A / all-T / all-N (:320-372)
	{
		const char bases[3] = {'A', 'T', 'N'}; const char *names[3] = {"allA.ids.bin", "allT.ids.bin", "allN.ids.bin"}; const long cnt[3] = {na, nt, nn};
		for (int q = 0; q < 3; ++q) {
			Ids ids; if (!slurp(dir + "/" + names[q], ids.b)) return -1;
			for (long i = 0; i < cnt[q]; ++i) { if (!ids.next(idx)) return -1; put(idx, std::string((size_t)L, bases[q])); }
		}
	}
	// near-constant reads (:374-493)
	{
		const char bases[3] = {'A', 'T', 'N'}; const char *names[3] = {"AA", "TT", "NN"};
		for (int q = 0; q < 3; ++q) {
			Ids ids;
			if (!slurp(dir + "/" + names[q] + ".txt", buf) || !slurp(dir + "/" + names[q] + ".ids.bin", ids.b)) return -1;
			const std::string cref((size_t)L, bases[q]);
			size_t s = 0;
			for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') {
				if (!decode_line((const char*)buf.data() + s, i - s, cref.c_str(), L, seq)) return -1;
				s = i + 1;
				if (!ids.next(idx)) return -1;
				put(idx, seq);
			}
		}
	}
	// unclustered reads (:238-280) and reads kept as text (:282-296)
	{
		Ids ids;
		if (!slurp(dir + "/single.seq", buf) || !slurp(dir + "/singleFile.ids.bin", ids.b)) return -1;
		DnaReader r(buf);
		for (;;) {
			seq.clear();
			int c = 0;
			for (int i = 0; i < L; ++i) { c = r.next(); if (c < 0) break; seq.push_back("ACGT"[c]); }
			if (c < 0 || (int)seq.size() < L) break;
			if (!ids.next(idx)) break;                                   // padding of the last byte can look like one more read of A
			put(idx, seq);
		}
		Ids nids;
		if (!slurp(dir + "/single_N.seq", buf) || !slurp(dir + "/Nfile.ids.bin", nids.b)) return -1;
		size_t s = 0;
		for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') { seq.assign((const char*)buf.data() + s, i - s); s = i + 1; if (!nids.next(idx)) return -1; put(idx, seq); }
	}
	// contigs (:109-236)
	for (int th = 0; th < nth; ++th) {
		std::vector<uint8_t> bref, bpos, bdir, bdif, bids;
		const std::string sfx = "." + std::to_string(th);
		if (!slurp(dir + "/ref.bin" + sfx, bref) || !slurp(dir + "/beg_pos.bin" + sfx, bpos) || !slurp(dir + "/dir.bin" + sfx, bdir) ||
		    !slurp(dir + "/dif_char.txt" + sfx, bdif) || !slurp(dir + "/ids.bin" + sfx, bids)) return -1;
		DnaReader rr(bref); BitReader dr(bdir);
		size_t pp = 0, dp = 0, ip = 0;
		std::string ref;
		uint64_t coff = 0;                                                  // bases of ref.bin before this contig (the agreement mask's places)
		if (agree) agree->L = L;
		while (pp + 4 <= bpos.size()) {
			uint32_t num; memcpy(&num, bpos.data() + pp, 4); pp += 4;
			ref.clear();
			int pre = 0; uint64_t pre_idx = 0;
			for (uint32_t q = 0; q < num; ++q) {
				if (pp + 2 > bpos.size() || ip + 4 > bids.size()) return -1;
				uint16_t d; memcpy(&d, bpos.data() + pp, 2); pp += 2;
				uint32_t v; memcpy(&v, bids.data() + ip, 4); ip += 4;
				uint64_t id = v;
				if (d == 0) id += pre_idx;                                 // same begin position: a difference (:178-181)
				pre_idx = id;
				const int pos = pre + d; pre = pos;
				while ((int)ref.size() < pos + L) { const int c = rr.next(); if (c < 0) return -1; ref.push_back("ACGT"[c]); }
				const int rev = dr.next();
				size_t e = dp; while (e < bdif.size() && bdif[e] != '\n') ++e;
				if (e >= bdif.size() || !decode_line((const char*)bdif.data() + dp, e - dp, ref.c_str() + pos, L, seq)) return -1;
				dp = e + 1;
				if (agree) agree->member(id & 0xFFFFFFFFull, coff + (uint64_t)pos, rev, seq.data(), ref.c_str() + pos);
				if (rev) revcomp(seq);
				put(id & 0xFFFFFFFFull, seq);
			}
			coff += ref.size();
		}
		if (agree) agree->end_set();
	}
	if (bad) return -1;
	for (uint8_t s : seen) if (!s) return -1;                              // every position filled exactly once
	if (keep) { keep->swap(table); if (L_out) *L_out = L; if (n_reads) *n_reads = n_seq; return 0; }
	FILE *out = fopen(out_path, "w");
	if (!out) return -1;
	for (size_t i = 0; i < n_seq; ++i) { fwrite(table.data() + i * (size_t)L, 1, (size_t)L, out); fputc('\n', out); }
	fclose(out);
	if (n_reads) *n_reads = n_seq;
	return 0;
}

// ---- paired end (_PE): decomp_AATTNN_pe (decompress.c:963-1212) + decompress_pe (:780-917) ----------------------------
// Reads of the first file are written to out_path1 in stream order (the eight lists, then the contig members); a read
// of the second file carries the line number of its mate (peids streams, one file bit per read says which kind a
// read is) and goes to that line of out_path2: line i of the two outputs is a pair.
// keep1 / keep2: the rows of the two files (L characters each) are handed out instead of being written (mcomh_decompress_fastq_pe)
static int decompress_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, std::vector<char> *keep1 = nullptr, std::vector<char> *keep2 = nullptr,
                              int *L_out = nullptr)
{
	const bool keep = keep1 && keep2;
	if (!folder || (!keep && (!out_path1 || !out_path2))) return -1;
	const std::string dir(folder);
	FILE *fi = fopen((dir + "/info.txt").c_str(), "r");
	if (!fi) return -1;
	int L = 0, nth = 0; long half = 0, na = 0, nt = 0, nn = 0;
	if (fscanf(fi, "%d %d %ld %ld %ld %ld", &L, &nth, &half, &na, &nt, &nn) != 6) { fclose(fi); return -1; }
	fclose(fi);
	if (L < 1 || L > 256 || nth < 1 || nth > 4096 || half < 0 || na < 0 || nt < 0 || nn < 0) return -1;
	{   // every read has one bit in a file.bin stream: the number of pairs cannot exceed what they hold
		size_t fbb = file_bytes(dir + "/file.bin.sp");
		for (int th = 0; th < nth; ++th) fbb += file_bytes(dir + "/file.bin." + std::to_string(th));
		if ((size_t)half > fbb * 8) return -1;
	}
	std::vector<char> table((size_t)half * (size_t)L, 0);
	std::vector<uint8_t> seen((size_t)half, 0);
	FILE *out = keep ? nullptr : fopen(out_path1, "w");
	if (!keep && !out) return -1;
	uint64_t left = 0; bool bad = false;
	struct Pairing {                                                      // file bits + mate numbers of one stream set
		std::vector<uint8_t> fb, ids; size_t ip = 0; size_t bpos = 0; int k = 8; unsigned cur = 0;
		int bit() { if (k >= 8) { cur = bpos < fb.size() ? fb[bpos++] : 0; k = 0; } const int c = (int)(cur & 1); cur >>= 1; ++k; return c; }
		bool id(uint32_t &v) { if (ip + 4 > ids.size()) return false; memcpy(&v, ids.data() + ip, 4); ip += 4; return true; }
	};
	auto place = [&](Pairing &pr, const std::string &s) {
		if ((int)s.size() != L) { bad = true; return; }
		if (pr.bit()) {                                                    // a read of the second file: to its mate's line
			uint32_t v; if (!pr.id(v) || v >= (uint64_t)half || seen[v]) { bad = true; return; }
			memcpy(table.data() + (size_t)v * L, s.data(), (size_t)L); seen[v] = 1;
		} else { if (keep) keep1->insert(keep1->end(), s.begin(), s.end()); else { fwrite(s.data(), 1, s.size(), out); fputc('\n', out); } ++left; }
	};
	std::vector<uint8_t> buf;
	std::string seq;
	Pairing sp;
	if (!slurp(dir + "/file.bin.sp", sp.fb) || !slurp(dir + "/peids.bin.sp", sp.ids)) { shut(out); return -1; }
	for (long i = 0; i < na; ++i) place(sp, std::string((size_t)L, 'A'));
	for (long i = 0; i < nt; ++i) place(sp, std::string((size_t)L, 'T'));
	for (long i = 0; i < nn; ++i) place(sp, std::string((size_t)L, 'N'));
	{
		const char bases[3] = {'A', 'T', 'N'}; const char *names[3] = {"AA.txt", "TT.txt", "NN.txt"};
		for (int q = 0; q < 3; ++q) {
			if (!slurp(dir + "/" + names[q], buf)) { shut(out); return -1; }
			const std::string cref((size_t)L, bases[q]);
			size_t s = 0;
			for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') { if (!decode_line((const char*)buf.data() + s, i - s, cref.c_str(), L, seq)) { shut(out); return -1; } s = i + 1; place(sp, seq); }
		}
	}
	if (!slurp(dir + "/single_N.seq", buf)) { shut(out); return -1; }
	{ size_t s = 0; for (size_t i = 0; i < buf.size(); ++i) if (buf[i] == '\n') { seq.assign((const char*)buf.data() + s, i - s); s = i + 1; place(sp, seq); } }
	if (!slurp(dir + "/single.seq", buf)) { shut(out); return -1; }
	{
		// the last byte may be padded with up to three A: reads are taken while whole reads remain (4 bases per byte)
		const size_t whole = buf.size() * 4 / (size_t)L;
		DnaReader r(buf);
		for (size_t i = 0; i < whole; ++i) {
			seq.clear();
			for (int j = 0; j < L; ++j) seq.push_back("ACGT"[r.next() & 3]);
			place(sp, seq);
		}
	}
	for (int th = 0; th < nth; ++th) {
		std::vector<uint8_t> bref, bpos, bdir, bdif;
		Pairing pr;
		const std::string sfx = "." + std::to_string(th);
		if (!slurp(dir + "/ref.bin" + sfx, bref) || !slurp(dir + "/beg_pos.bin" + sfx, bpos) || !slurp(dir + "/dir.bin" + sfx, bdir) ||
		    !slurp(dir + "/dif_char.txt" + sfx, bdif) || !slurp(dir + "/file.bin" + sfx, pr.fb) || !slurp(dir + "/peids.bin" + sfx, pr.ids)) { shut(out); return -1; }
		DnaReader rr(bref); BitReader dr(bdir);
		size_t pp = 0, dp = 0;
		std::string ref;
		while (pp + 4 <= bpos.size()) {
			uint32_t num; memcpy(&num, bpos.data() + pp, 4); pp += 4;
			ref.clear();
			int pre = 0;
			for (uint32_t q = 0; q < num; ++q) {
				if (pp + 2 > bpos.size()) { shut(out); return -1; }
				uint16_t d; memcpy(&d, bpos.data() + pp, 2); pp += 2;
				const int pos = pre + d; pre = pos;
				while ((int)ref.size() < pos + L) { const int c = rr.next(); if (c < 0) { shut(out); return -1; } ref.push_back("ACGT"[c]); }
				const int rev = dr.next();
				size_t e = dp; while (e < bdif.size() && bdif[e] != '\n') ++e;
				if (e >= bdif.size() || !decode_line((const char*)bdif.data() + dp, e - dp, ref.c_str() + pos, L, seq)) { shut(out); return -1; }
				dp = e + 1;
				if (rev) revcomp(seq);
				place(pr, seq);
			}
		}
	}
	shut(out);
	if (bad || left != (uint64_t)half) return -1;
	for (uint8_t s : seen) if (!s) return -1;
	if (keep) { keep2->swap(table); if (L_out) *L_out = L; if (n_pairs) *n_pairs = (uint64_t)half; return 0; }
	FILE *out2 = fopen(out_path2, "w");
	if (!out2) return -1;
	for (long i = 0; i < half; ++i) { fwrite(table.data() + (size_t)i * L, 1, (size_t)L, out2); fputc('\n', out2); }
	fclose(out2);
	if (n_pairs) *n_pairs = (uint64_t)half;
	return 0;
}

// no C++ exception crosses the C boundary (a corrupt info.txt can ask for more memory than there is)
extern "C" int mcomh_decompress(const char *folder, const char *out_path, uint64_t *n_reads)
{
	try { return decompress_impl(folder, out_path, n_reads); } catch (...) { return -1; }
}

// ---- a ragged archive (`minicom -p -V`): folder/len.bin says which records are the core's reads of L bases and
// which lie in odd.seq / odd.qual.  The core's reads (and qual.mcq's rows) are decoded as ever, then the records are laid out in input
// order by mcomh_fastq_emit_ragged: one read per line, or -- fastq -- four-line records named by name.mcn or `@<i+1>`.  A folder whose
// parts disagree is refused and no file is written.
static int decompress_ragged_impl(const char *folder, const char *out_path, uint64_t *n_reads, bool fastq)
{
	if (!folder || !out_path) return -1;
	std::vector<char> reads; int L = 0; uint64_t n_even = 0;
	if (decompress_order_impl(folder, nullptr, &n_even, &reads, &L)) return -1;
	std::vector<uint8_t> qmember, nmember, quals, names;
	const bool has_qual = slurp(std::string(folder) + "/qual.mcq", qmember), named = slurp(std::string(folder) + "/name.mcn", nmember);
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
	std::vector<uint64_t> rec_off;
	if (fastq) {
		quals.resize((size_t)n_even * (size_t)L + 1);
		if (mcomh_qual_decode(qmember.data(), qmember.size(), quals.data(), (uint64_t)L, n_even, &qn, &qL) || qn != n_even || (int)qL != L) return -1;
		S.quals = quals.data(); S.qual_pitch = (uint64_t)L; S.odd_qual = P.odd_qual.data();
		if (named) {
			names.resize(tl + 1);
			if (mcomh_name_decode(nmember.data(), nmember.size(), names.data(), tl, &tl, &nn) || nn != P.n) return -1;
			rec_off.reserve(P.n + 1); rec_off.push_back(0);
			uint64_t lines = 0;
			for (uint64_t i = 0; i < tl; ++i) if (names[i] == '\n' && (++lines & 1) == 0) rec_off.push_back(i + 1);
			if (lines != 2 * P.n || rec_off.size() != P.n + 1) return -1;
			S.names = names.data(); S.names_bytes = tl; S.rec_off = rec_off.data();
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

// no C++ exception crosses the C boundary (a corrupt info.txt can ask for more memory than there is)
extern "C" int mcomh_decompress_order(const char *folder, const char *out_path, uint64_t *n_reads)
{
	try { return folder && mcom_ragged_present(folder) ? decompress_ragged_impl(folder, out_path, n_reads, false) : decompress_order_impl(folder, out_path, n_reads); } catch (...) { return -1; }
}

// no C++ exception crosses the C boundary (a corrupt info.txt can ask for more memory than there is)
extern "C" int mcomh_decompress_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	try { return decompress_pe_impl(folder, out_path1, out_path2, n_pairs); } catch (...) { return -1; }
}

// ---- a -p -Q archive back to FASTQ on the host: the reads of decompress_order_impl in memory, the quality
// rows of folder/qual.mcq by the host twin, then records `@<i+1>`, read, `+`, qualities.  The cross-check of mcomh_decompress_fastq_gpu:
// the same bytes, the same archives refused (one that is not a -p archive, no qual.mcq, another n or L than the reads).  With
// folder/name.mcn (section 3.10) the records are `@<name>`, read, `+<text>`, qualities; a name.mcn of another n or a refused one is an error.
static int decompress_fastq_impl(const char *folder, const char *out_path, uint64_t *n_reads)
{
	if (!folder || !out_path) return -1;
	std::vector<char> reads; int L = 0; uint64_t n = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L)) return -1;
	std::vector<uint8_t> member;
	if (!slurp(std::string(folder) + "/qual.mcq", member)) return -1;
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcomh_qual_info(member.data(), member.size(), &qn, &qL) || qn != n || (int)qL != L) return -1;
	std::vector<uint8_t> quals((size_t)n * (size_t)L + 1);
	if (mcomh_qual_decode(member.data(), member.size(), quals.data(), (uint64_t)L, n, &qn, &qL) || qn != n || (int)qL != L) return -1;
	// folder/name.mcn (`minicom -N`, section 3.10): the records carry its names and '+' texts; it must state the reads' number
	std::vector<uint8_t> names; std::vector<uint64_t> name_at;
	std::vector<uint8_t> nmember;
	const bool named = slurp(std::string(folder) + "/name.mcn", nmember);
	if (named) {
		uint64_t nn = 0, tl = 0;
		if (mcomh_name_info(nmember.data(), nmember.size(), &nn, &tl) || nn != n) return -1;
		names.resize(tl + 1);
		if (mcomh_name_decode(nmember.data(), nmember.size(), names.data(), tl, &tl, &nn) || nn != n) return -1;
		name_at.reserve(2 * n + 1); name_at.push_back(0);
		for (uint64_t i = 0; i < tl; ++i) if (names[i] == '\n') name_at.push_back(i + 1);
		if (name_at.size() != 2 * n + 1) return -1;
	}
	FILE *out = fopen(out_path, "wb");
	if (!out) return -1;
	bool ok = true;
	for (uint64_t i = 0; i < n && ok; ++i) {
		if (named) {
			const uint64_t a = name_at[2 * i], b = name_at[2 * i + 1], c = name_at[2 * i + 2];
			ok = fputc('@', out) != EOF && fwrite(names.data() + a, 1, b - a, out) == b - a && fwrite(reads.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputs("\n+", out) >= 0 &&
			     fwrite(names.data() + b, 1, c - b, out) == c - b;
		} else
			ok = fprintf(out, "@%llu\n", (unsigned long long)(i + 1)) > 0 && fwrite(reads.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputs("\n+\n", out) >= 0;
		ok = ok && fwrite(quals.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
	}
	if (fclose(out) != 0 || !ok) { remove(out_path); return -1; }
	if (n_reads) *n_reads = n;
	return 0;
}

extern "C" int mcomh_decompress_fastq(const char *folder, const char *out_path, uint64_t *n_reads)
{
	try { return folder && mcom_ragged_present(folder) ? decompress_ragged_impl(folder, out_path, n_reads, true) : decompress_fastq_impl(folder, out_path, n_reads); } catch (...) { return -1; }
}

// ---- `minicom -q` archives back to FASTQ on the host: the rows of the default / paired-end decoder in memory,
// the quality rows of folder/rqual.mcq (paired end: rqual_1.mcq and rqual_2.mcq) by the host twin -- they are stored in the archive's
// own order, row j beside read j -- then records `@<j+1>`, read, `+`, qualities.  The cross-check of the _gpu routes: the same bytes,
// the same archives refused (-p archives, an archive of the other kind, a missing member, one of another n or L than the reads, a
// refused member); no output file is left then.
namespace {
bool exists(const std::string &path) { FILE *f = fopen(path.c_str(), "rb"); if (!f) return false; fclose(f); return true; }

bool load_quals(const std::string &path, uint64_t n, int L, std::vector<uint8_t> &quals)
{
	std::vector<uint8_t> member;
	if (!slurp(path, member)) return false;
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcomh_qual_info(member.data(), member.size(), &qn, &qL) || qn != n || (int)qL != L) return false;
	quals.assign((size_t)n * (size_t)L + 1, 0);
	return !mcomh_qual_decode(member.data(), member.size(), quals.data(), (uint64_t)L, n, &qn, &qL) && qn == n && (int)qL == L;
}

bool write_records(const char *path, const std::vector<char> &reads, const std::vector<uint8_t> &quals, uint64_t n, int L)
{
	FILE *out = fopen(path, "wb");
	if (!out) return false;
	bool ok = true;
	for (uint64_t i = 0; i < n && ok; ++i)
		ok = fprintf(out, "@%llu\n", (unsigned long long)(i + 1)) > 0 && fwrite(reads.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputs("\n+\n", out) >= 0 &&
		     fwrite(quals.data() + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
	if (fclose(out) != 0 || !ok) { remove(path); return false; }
	return true;
}
}  // namespace

static int decompress_fastq_reordered_impl(const char *folder, const char *out_path, uint64_t *n_reads)
{
	if (!folder || !out_path) return -1;
	const std::string dir(folder);
	if (exists(dir + "/allA.ids.bin") || exists(dir + "/file.bin.sp")) return -1;      // a -p or a paired-end archive
	std::vector<char> reads; int L = 0; uint64_t n = 0;
	if (decompress_impl(folder, nullptr, &n, &reads, &L)) return -1;
	std::vector<uint8_t> quals;
	if (!load_quals(dir + "/rqual.mcq", n, L, quals)) return -1;
	if (!write_records(out_path, reads, quals, n, L)) return -1;
	if (n_reads) *n_reads = n;
	return 0;
}

static int decompress_fastq_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	const std::string dir(folder);
	if (exists(dir + "/allA.ids.bin")) return -1;                                       // a -p archive
	std::vector<char> r1, r2; int L = 0; uint64_t n = 0;
	if (decompress_pe_impl(folder, nullptr, nullptr, &n, &r1, &r2, &L)) return -1;
	std::vector<uint8_t> q1, q2;
	if (!load_quals(dir + "/rqual_1.mcq", n, L, q1) || !load_quals(dir + "/rqual_2.mcq", n, L, q2)) return -1;
	if (!write_records(out_path1, r1, q1, n, L)) return -1;
	if (!write_records(out_path2, r2, q2, n, L)) { remove(out_path1); return -1; }
	if (n_pairs) *n_pairs = n;
	return 0;
}

extern "C" int mcomh_decompress_fastq_reordered(const char *folder, const char *out_path, uint64_t *n_reads)
{
	try { return decompress_fastq_reordered_impl(folder, out_path, n_reads); } catch (...) { return -1; }
}

extern "C" int mcomh_decompress_fastq_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	try { return decompress_fastq_pe_impl(folder, out_path1, out_path2, n_pairs); } catch (...) { return -1; }
}

// ---- a pair kept in input order (`minicom -1 -2 -p [-Q [-N]]`) on the host: the 2 n rows of decompress_order_impl,
// rows [0, n) to the first file and [n, 2 n) to the second.  folder/pe_order.txt (one line, n) must agree with the reads' number.  With
// quality values: qual_1.mcq and qual_2.mcq, n rows each; with names: name_1.mcn (kind 0 or 1) and name_2.mcn, which is decoded with the
// decoded name_1 text as its mate.  The cross-check of the _gpu routes: the same bytes, the same archives refused; neither file is left.
namespace {
// n_pairs of folder/pe_order.txt, which must be half of n_rows
bool pair_count(const std::string &dir, uint64_t n_rows, uint64_t &n_pairs)
{
	std::vector<uint8_t> t;
	if (!slurp(dir + "/pe_order.txt", t) || t.empty() || t.size() > 24 || t.back() != '\n') return false;
	uint64_t v = 0;
	for (size_t i = 0; i + 1 < t.size(); ++i) { if (t[i] < '0' || t[i] > '9') return false; v = v * 10 + (uint64_t)(t[i] - '0'); }
	n_pairs = v;
	return t.size() > 1 && (n_rows & 1) == 0 && v == n_rows / 2;
}
struct NameText { std::vector<uint8_t> text; std::vector<uint64_t> at; uint64_t len = 0; };
bool index_names(NameText &t, uint64_t n)
{
	t.at.clear(); t.at.reserve(2 * n + 1); t.at.push_back(0);
	for (uint64_t i = 0; i < t.len; ++i) if (t.text[i] == '\n') t.at.push_back(i + 1);
	return t.at.size() == 2 * n + 1;
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

static int decompress_order_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	std::vector<char> reads; int L = 0; uint64_t n = 0, half = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L)) return -1;
	if (!pair_count(folder, n, half)) return -1;
	const char *paths[2] = {out_path1, out_path2};
	for (int k = 0; k < 2; ++k) {
		FILE *out = fopen(paths[k], "wb");
		bool ok = out != nullptr;
		for (uint64_t i = 0; i < half && ok; ++i) ok = fwrite(reads.data() + ((uint64_t)k * half + i) * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
		if (out && fclose(out) != 0) ok = false;
		if (!ok) { remove(out_path1); remove(out_path2); return -1; }
	}
	if (n_pairs) *n_pairs = half;
	return 0;
}

static int decompress_fastq_order_pe_impl(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	if (!folder || !out_path1 || !out_path2) return -1;
	const std::string dir(folder);
	std::vector<char> reads; int L = 0; uint64_t n = 0, half = 0;
	if (decompress_order_impl(folder, nullptr, &n, &reads, &L)) return -1;
	if (!pair_count(dir, n, half)) return -1;
	std::vector<uint8_t> q[2];
	if (!load_quals(dir + "/qual_1.mcq", half, L, q[0]) || !load_quals(dir + "/qual_2.mcq", half, L, q[1])) return -1;
	NameText nm[2];
	std::vector<uint8_t> m1, m2;
	const bool has1 = slurp(dir + "/name_1.mcn", m1), has2 = slurp(dir + "/name_2.mcn", m2);
	if (has1 != has2) return -1;                                                        // name_2 is coded against name_1; one alone is no archive
	if (has1) {
		uint64_t nn = 0, tl = 0;
		if (mcomh_name_info(m1.data(), m1.size(), &nn, &tl) || nn != half) return -1;
		nm[0].text.resize(tl + 1);
		if (mcomh_name_decode(m1.data(), m1.size(), nm[0].text.data(), tl, &tl, &nn) || nn != half) return -1;
		nm[0].len = tl;
		if (mcomh_name_info_mate(m2.data(), m2.size(), &nn, &tl) || nn != half) return -1;
		nm[1].text.resize(tl + 1);
		if (mcomh_name_decode_mate(m2.data(), m2.size(), nm[0].text.data(), nm[0].len, nm[1].text.data(), tl, &tl, &nn) || nn != half) return -1;
		nm[1].len = tl;
		if (!index_names(nm[0], half) || !index_names(nm[1], half)) return -1;
	}
	if (!write_records_named(out_path1, reads.data(), q[0], has1 ? &nm[0] : nullptr, half, L)) return -1;
	if (!write_records_named(out_path2, reads.data() + half * (size_t)L, q[1], has1 ? &nm[1] : nullptr, half, L)) { remove(out_path1); return -1; }
	if (n_pairs) *n_pairs = half;
	return 0;
}

extern "C" int mcomh_decompress_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	try { return decompress_order_pe_impl(folder, out_path1, out_path2, n_pairs); } catch (...) { return -1; }
}

extern "C" int mcomh_decompress_fastq_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs)
{
	try { return decompress_fastq_order_pe_impl(folder, out_path1, out_path2, n_pairs); } catch (...) { return -1; }
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

// the rows [first, first + count) of a quality member that must state n rows of L bytes
bool load_quals_rows(const std::string &path, uint64_t n, int L, uint64_t first, uint64_t count, std::vector<uint8_t> &quals)
{
	std::vector<uint8_t> member;
	if (!slurp(path, member)) return false;
	uint64_t qn = 0; uint32_t qL = 0;
	if (mcomh_qual_info(member.data(), member.size(), &qn, &qL) || qn != n || (int)qL != L) return false;
	quals.assign((size_t)count * (size_t)L + 1, 0);
	return !mcomh_qual_decode_rows(member.data(), member.size(), first, count, quals.data(), (uint64_t)L, &qn, &qL) && qn == n && (int)qL == L;
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
	const int n_files = pair ? 2 : 1;
	const char *paths[2] = {out_path1, out_path2};
	std::vector<uint8_t> q[2];
	NameText nm[2];
	bool named = false;
	if (fastq) {
		const char *qname[2] = {pair ? "/qual_1.mcq" : "/qual.mcq", "/qual_2.mcq"}, *nname[2] = {pair ? "/name_1.mcn" : "/name.mcn", "/name_2.mcn"};
		for (int k = 0; k < n_files; ++k) if (!load_quals_rows(dir + qname[k], n, L, first, count, q[k])) { fprintf(stderr, "minicom decoder: %s%s is missing, refused or states another number or length than the reads\n", folder, qname[k]); return -1; }
		std::vector<uint8_t> m[2];
		const bool has1 = slurp(dir + nname[0], m[0]), has2 = pair && slurp(dir + nname[1], m[1]);
		if (pair && has1 != has2) return -1;                                    // name_2 is coded against name_1; one alone is no archive
		named = has1;
		for (int k = 0; k < n_files && named; ++k) {
			uint64_t nn = 0, tl = 0;
			if ((k ? mcomh_name_info_mate(m[k].data(), m[k].size(), &nn, &tl) : mcomh_name_info(m[k].data(), m[k].size(), &nn, &tl)) || nn != n) return -1;
			nm[k].text.resize(tl + 1);
			if ((k ? mcomh_name_decode_mate(m[k].data(), m[k].size(), nm[0].text.data(), nm[0].len, nm[k].text.data(), tl, &tl, &nn)
			       : mcomh_name_decode(m[k].data(), m[k].size(), nm[k].text.data(), tl, &tl, &nn)) || nn != n) return -1;
			nm[k].len = tl;
			if (!index_names(nm[k], n)) return -1;
		}
	}
	for (int k = 0; k < n_files; ++k) {
		const char *rows = reads.data() + ((uint64_t)k * n + first) * (size_t)L;
		bool ok;
		if (fastq) ok = write_records_named(paths[k], rows, q[k], named ? &nm[k] : nullptr, count, L, first);
		else {
			FILE *out = fopen(paths[k], "wb");
			ok = out != nullptr;
			for (uint64_t i = 0; i < count && ok; ++i) ok = fwrite(rows + i * (size_t)L, 1, (size_t)L, out) == (size_t)L && fputc('\n', out) != EOF;
			if (out && fclose(out) != 0) ok = false;
		}
		if (!ok) { for (int j = 0; j <= k; ++j) remove(paths[j]); return -1; }
	}
	if (n_written) *n_written = count;
	return 0;
}

int range_any(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, int device, bool pair, bool fastq)
{
	if (!folder || !out_path1 || (pair && !out_path2)) return -1;
	if (const char *why = range_refusal(folder)) { fprintf(stderr, "minicom decoder: a range of %s is refused: %s\n", folder, why); return -1; }
	try {
		if (device < 0) return range_host(folder, out_path1, out_path2, first, count, n_written, pair, fastq);
#ifdef MCOM_ENTROPY_HOST_ONLY
		fprintf(stderr, "minicom decoder: this build has no GPU route\n");
		return -1;
#else
		return mcom_range_gpu(folder, out_path1, out_path2, first, count, n_written, device, pair, fastq);
#endif
	} catch (...) { return -1; }   // no C++ exception crosses the C boundary
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
	try {
		McomAgreeSink sink; sink.C = C;
		std::vector<char> reads; int L = 0; uint64_t n = 0;
		if (order ? decompress_order_impl(folder, nullptr, &n, &reads, &L, &sink) : decompress_impl(folder, nullptr, &n, &reads, &L, &sink)) return -1;
		const size_t mb = (size_t)(L + 7) / 8;
		mask.assign((size_t)n * mb, 0);
		for (const McomAgreeSink::Row &r : sink.rows) { if (r.row >= n) return -1; memcpy(mask.data() + (size_t)r.row * mb, r.bits, mb); }
		if (n_rows) *n_rows = n;
		if (L_out) *L_out = L;
		return 0;
	} catch (...) { return -1; }
}
