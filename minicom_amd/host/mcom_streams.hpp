// minicom_amd/host/mcom_streams.hpp -- what a folder of stream files holds in each of the three modes: the one statement of it, read by the
// host decoder (mcom_decompress.cpp: one section or stream set in memory at a time) and by the GPU decoder (mcom_decompress_gpu.cpp: all of
// them, uploaded whole).  info.txt and its bounds, the file names per mode, the loaders, and the size checks that keep a corrupt info.txt
// from asking for memory.  Header only, internal to libmcom_host.
#pragma once
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

namespace mcom_streams {

enum Mode { DEFAULT = 0, ORDER = 1, PE = 2 };             // as written / -p: every stream has a companion stream of read ids / paired end
struct StreamInfo { int L = 0, nth = 0; long na = 0, nt = 0, nn = 0, half = 0; unsigned long n_seq = 0; };

inline bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
	if (n < 0) { fclose(f); return false; }
	out.resize((size_t)n);
	size_t got = n ? fread(out.data(), 1, (size_t)n, f) : 0;
	fclose(f);
	return got == (size_t)n;
}
inline bool exists(const std::string &path) { FILE *f = fopen(path.c_str(), "rb"); if (!f) return false; fclose(f); return true; }
inline size_t file_bytes(const std::string &path)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return 0;
	fseek(f, 0, SEEK_END); const long n = ftell(f); fclose(f);
	return n > 0 ? (size_t)n : 0;
}

// info.txt: L, the number of stream sets (writer threads), the counted all-A / all-T / all-N reads; -p: and n_seq, paired end: and half
inline bool read_info(Mode mode, const std::string &dir, StreamInfo &I)
{
	FILE *fi = fopen((dir + "/info.txt").c_str(), "r");
	if (!fi) return false;
	const int want = mode == DEFAULT ? 5 : 6;
	const int got = mode == DEFAULT ? fscanf(fi, "%d %d %ld %ld %ld", &I.L, &I.nth, &I.na, &I.nt, &I.nn)
	              : mode == ORDER   ? fscanf(fi, "%d %d %ld %ld %ld %lu", &I.L, &I.nth, &I.na, &I.nt, &I.nn, &I.n_seq)
	                                : fscanf(fi, "%d %d %ld %ld %ld %ld", &I.L, &I.nth, &I.half, &I.na, &I.nt, &I.nn);
	fclose(fi);
	return got == want && I.L >= 1 && I.L <= 256 && I.nth >= 1 && I.nth <= 4096 && I.na >= 0 && I.nt >= 0 && I.nn >= 0 && I.half >= 0;
}

// ---- the eight sections in front of the stream sets, in the order they are walked; -p: each with its list of read ids
enum Kind { COUNTED, NEAR, VERBATIM, PACKED };            // reads that are only counted | text against a constant base | lines as they are | 2 bits per base
struct Section { Kind kind; char base; const char *data, *ids; };
const int N_SECTIONS = 8;
const Section SECTIONS[N_SECTIONS] = {
	{COUNTED, 'A', nullptr, "allA.ids.bin"}, {COUNTED, 'T', nullptr, "allT.ids.bin"}, {COUNTED, 'N', nullptr, "allN.ids.bin"},
	{NEAR, 'A', "AA.txt", "AA.ids.bin"}, {NEAR, 'T', "TT.txt", "TT.ids.bin"}, {NEAR, 'N', "NN.txt", "NN.ids.bin"},
	{VERBATIM, 'N', "single_N.seq", "Nfile.ids.bin"}, {PACKED, 0, "single.seq", "singleFile.ids.bin"}};
struct SectionFiles { std::vector<uint8_t> data, ids; };
inline bool load_section(Mode mode, const std::string &dir, int s, SectionFiles &f)
{
	return (!SECTIONS[s].data || slurp(dir + "/" + SECTIONS[s].data, f.data)) && (mode != ORDER || slurp(dir + "/" + SECTIONS[s].ids, f.ids));
}

// ---- one stream set per writer thread, suffix .<th>; paired end: file bits and mate numbers per set, and one pair (.sp) for all sections
struct SetFiles { std::vector<uint8_t> ref, pos, dir, dif, ids, fb, pe; };
inline bool load_pairing(const std::string &dir, const std::string &sfx, SetFiles &f) { return slurp(dir + "/file.bin" + sfx, f.fb) && slurp(dir + "/peids.bin" + sfx, f.pe); }
inline bool load_set(Mode mode, const std::string &dir, int th, SetFiles &f)
{
	const std::string sfx = "." + std::to_string(th);
	return slurp(dir + "/ref.bin" + sfx, f.ref) && slurp(dir + "/beg_pos.bin" + sfx, f.pos) && slurp(dir + "/dir.bin" + sfx, f.dir) && slurp(dir + "/dif_char.txt" + sfx, f.dif) &&
	       (mode != ORDER || slurp(dir + "/ids.bin" + sfx, f.ids)) && (mode != PE || load_pairing(dir, sfx, f));
}

// The first size checks, made before a table of n_seq x L or half x L bytes is asked for.  -p: every read has a 4-byte entry in one of the
// id streams, n_seq cannot exceed what they hold; paired end: every read has one bit in a file.bin stream, and so has every pair.
inline bool counts_fit(Mode mode, const std::string &dir, const StreamInfo &I)
{
	if (mode == DEFAULT) return true;
	size_t bytes = mode == PE ? file_bytes(dir + "/file.bin.sp") : 0;
	for (int s = 0; s < N_SECTIONS && mode == ORDER; ++s) bytes += file_bytes(dir + "/" + SECTIONS[s].ids);
	for (int th = 0; th < I.nth; ++th) bytes += file_bytes(dir + (mode == ORDER ? "/ids.bin." : "/file.bin.") + std::to_string(th));
	return mode == ORDER ? (size_t)I.n_seq <= bytes / 4 : (size_t)I.half <= bytes * 8;
}

// folder/pe_order.txt of a pair kept in input order (`minicom -1 -2 -p`): one line, n_pairs, which must be half of n_rows
inline bool pair_count(const std::string &dir, uint64_t n_rows, uint64_t &n_pairs)
{
	std::vector<uint8_t> t;
	if (!slurp(dir + "/pe_order.txt", t) || t.empty() || t.size() > 24 || t.back() != '\n') return false;
	uint64_t v = 0;
	for (size_t i = 0; i + 1 < t.size(); ++i) { if (t[i] < '0' || t[i] > '9') return false; v = v * 10 + (uint64_t)(t[i] - '0'); }
	n_pairs = v;
	return t.size() > 1 && (n_rows & 1) == 0 && v == n_rows / 2;
}

}  // namespace mcom_streams
