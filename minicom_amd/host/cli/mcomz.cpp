// mcomz e|d [--gpu] [--bwt] IN OUT -- the built-in entropy stage as a program: it stands where the reference's script runs `bsc e IN OUT`
// and `bsc d IN OUT` (minicom:115, :346).  e: IN -> a `.rans` member, with --bwt a `.bwt` member (the block-sorting coder, DESIGN.md
// section 3.8); d: the way back, the kind of member taken from its first four bytes.  Host twin by default, GPU 0 with --gpu (an error,
// not the host twin, when there is none).  Exit status 1 and no output file when IN cannot be read, is not a complete, intact member, or
// OUT cannot be written.
// mcomz e --qual L [--gpu] IN OUT: IN is n * L raw quality bytes (row after row), OUT a `.mcq` member; d knows
// such a member by its magic and writes the raw bytes back.
// mcomz e --fastq-qual L [--gpu] IN.fastq OUT: the quality lines of a four-line FASTQ file (plain or .gz) of reads of L bases -> a `.mcq`
// member; every record is checked ('@' line, '+' line, both lengths, quality bytes 33 .. 126) and the first bad one is named -- on the
// GPU by the kernels behind mcomh_fastq_qualities_to_device, without --gpu by their host twin.  Prints the number of records.
// mcomz e --fastq-qual L --order FILE [--gpu] IN.fastq OUT: the same with row j of the member = record order[j] of IN.fastq, FILE holding
// one little-endian u32 per record (read_order.bin of `minicom -q`); exit status 1 and no member when FILE is
// no permutation of the records (its size, its entry count, an entry beyond the last record, a record named twice).
// mcomz e --qual L --lossy SPEC, mcomz e --fastq-qual L [--order FILE] --lossy SPEC: the rows go through the lossy transform SPEC (ill8,
// thr:T:LO:HI or pblock:P in their canonical form) in front of the coder -- mcom_qual_transform with --gpu, its host
// twin without, the same member either way.  The report goes to stderr in one line, `lossy SPEC: changed C sum_abs A sum_sq S max_abs M`;
// a spec the parser refuses is exit status 1 and no member.  pblock is not idempotent: coding a decoded matrix again changes it again.
// mcomz e --fastq-qual L [--order FILE] --agree Q MASKFILE [--mask-first ROW] [--lossy SPEC]: the rows go through the agreement transform of
// `minicom -a` behind the gather and in front of SPEC: the value of every column whose bit of MASKFILE
// (`decompress --agree-mask`) is set becomes Phred Q; row r of the member belongs to mask row ROW + r (ROW 0 without --mask-first).  The
// report goes to stderr in one line, `agree Q: mask_bits B changed C sum_abs A sum_sq S max_abs M`, in front of the lossy one.
// mcomz e / d take `odd.aln` (`minicom -p -V -A`) as any other side member: it is made by `decompress --odd-align`,
// not here, and is packed with len.bin, odd.seq and odd.qual through the codec the archive's other members go through.
// mcomz --lossy-spec SPEC: prints the canonical text of SPEC; exit status 1 when the parser refuses it (what `minicom -b` asks first).
// mcomz e --names [--gpu] IN OUT: IN is a name text (per record its name and the text of its third line, a line each; DESIGN.md section
// 3.10), OUT a `.mcn` member; a line above 255 bytes is refused and its record named.  d knows such a member by its magic.
// mcomz e --fastq-names [--gpu] IN.fastq OUT: the names and '+' texts of a four-line FASTQ file (plain or .gz) -> a `.mcn` member; every
// record is checked ('@' line, '+' line, at most 255 bytes behind either) and the first bad one is named.  Prints the number of records.
// mcomz e --names --mate TEXT1 [--gpu] IN OUT, mcomz e --fastq-names --mate FILE_1.fastq [--gpu] IN.fastq OUT, mcomz d --mate TEXT1 IN OUT:
// IN is the second file of a pair and the mate the first; the member is coded against the mate's names where that is smaller (kind 2,
// DESIGN.md section 3.12), and d --mate gives the text back from a `.mcn` member of any kind (exit status 1 for a member of another
// coder: --mate has no meaning there).  d without --mate refuses a kind-2 member.
// mcomz z [--gpu] IN OUT.gz: IN as a BGZF file (gzip members of 65280 bytes of text each and the empty last member, DESIGN.md section
// 3.14) -- mcom_bgzf_encode with --gpu, its host twin without, the same file either way.  What `minicom -d -z` runs without -G.
// mcomz u [--gpu] IN.gz OUT: the inverse of z, a BGZF file to its text -- mcom_gzip_inflate with --gpu, its host
// twin without.  Exit status 1 and no OUT when a member is refused or IN.gz is not BGZF members to its end.
// mcomz e --fastq-lengths [--gpu] IN.fastq OUT: the first pass of `minicom -p -V`: OUT is len.bin, one byte
// (length - 1) per record; prints `n L n_odd` -- the records, the modal length, the records of another length.
// mcomz e --fastq-qual L --ragged LENFILE [--gpu] IN.fastq OUT.mcq OUT.oddqual: the `.mcq` member over the records of L bases and the
// quality lines of the others back to back; prints the number of rows of the member.
// mcomz e --fastq-digest [--gpu] [--no-qual] IN.fastq [IN_2.fastq] OUT: the digest of `minicom -K` of one file or of a
// pair as digest.txt; --no-qual leaves the quality keys out (what -K passes beside -b and -a).  Prints the number of records per file.
// Exit status 1, no OUT and a message that says why for a file that is not four-line records, or a pair of different record counts.
#include "../../../include/mcom_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool has_magic(const char *path, const char *magic4)
{
	char magic[4] = {0, 0, 0, 0};
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	const bool got = fread(magic, 1, 4, f) == 4;
	fclose(f);
	return got && !memcmp(magic, magic4, 4);
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "--lossy-spec")) {
		mcomh_qual_lossy_spec sp; char text[32];
		if (mcomh_qual_lossy_parse(argv[2], &sp) || mcomh_qual_lossy_print(&sp, text, sizeof text)) return 1;
		printf("%s\n", text);
		return 0;
	}
	if (argc > 1 && !strcmp(argv[1], "z")) {
		const bool z_gpu = argc == 5 && !strcmp(argv[2], "--gpu");
		if (argc != (z_gpu ? 5 : 4)) { fprintf(stderr, "usage: mcomz z [--gpu] IN OUT.gz\n"); return 1; }
		const char *z_in = argv[argc - 2], *z_out = argv[argc - 1];
		if (mcomh_bgzf_file(z_in, z_out, z_gpu ? 0 : -1)) {
			fprintf(stderr, "mcomz: cannot write %s as BGZF to %s%s\n", z_in, z_out, z_gpu ? " (or the GPU route is not available)" : "");
			return 1;
		}
		return 0;
	}
	if (argc > 1 && !strcmp(argv[1], "u")) {
		const bool u_gpu = argc == 5 && !strcmp(argv[2], "--gpu");
		if (argc != (u_gpu ? 5 : 4)) { fprintf(stderr, "usage: mcomz u [--gpu] IN.gz OUT\n"); return 1; }
		const char *u_in = argv[argc - 2], *u_out = argv[argc - 1];
		if (mcomh_gunzip_file(u_in, u_out, u_gpu ? 0 : -1)) {
			fprintf(stderr, "mcomz: %s is not a BGZF file of intact members, or %s cannot be written%s\n", u_in, u_out, u_gpu ? " (or the GPU route is not available)" : "");
			return 1;
		}
		return 0;
	}
	// the two passes of `minicom -p -V` that are not the core's
	if (argc > 2 && !strcmp(argv[1], "e") && !strcmp(argv[2], "--fastq-lengths")) {
		const bool l_gpu = argc == 6 && !strcmp(argv[3], "--gpu");
		if (argc != (l_gpu ? 6 : 5)) { fprintf(stderr, "usage: mcomz e --fastq-lengths [--gpu] IN.fastq OUT\n"); return 1; }
		char err[320] = ""; uint64_t n = 0, n_odd = 0; int L = 0;
		if (mcomh_fastq_lengths_file(argv[argc - 2], l_gpu ? 0 : -1, 0, argv[argc - 1], &n, &L, &n_odd, err, sizeof err)) { fprintf(stderr, "mcomz: %s: %s\n", argv[argc - 2], err[0] ? err : "cannot take the lengths"); return 1; }
		printf("%llu %d %llu\n", (unsigned long long)n, L, (unsigned long long)n_odd);
		return 0;
	}
	if (argc > 5 && !strcmp(argv[1], "e") && !strcmp(argv[2], "--fastq-qual") && !strcmp(argv[4], "--ragged")) {
		const bool r_gpu = argc == 10 && !strcmp(argv[6], "--gpu");
		const int r_L = atoi(argv[3]);
		if (argc != (r_gpu ? 10 : 9) || r_L < 1 || r_L > 256) { fprintf(stderr, "usage: mcomz e --fastq-qual L --ragged LENFILE [--gpu] IN.fastq OUT.mcq OUT.oddqual\n"); return 1; }
		char err[320] = ""; uint64_t n_even = 0;
		if (mcomh_fastq_quality_member_ragged(argv[argc - 3], r_L, r_gpu ? 0 : -1, argv[5], argv[argc - 2], argv[argc - 1], &n_even, err, sizeof err)) {
			fprintf(stderr, "mcomz: %s: %s\n", argv[argc - 3], err[0] ? err : "cannot code the qualities"); return 1;
		}
		printf("%llu\n", (unsigned long long)n_even);
		return 0;
	}
	if (argc > 2 && !strcmp(argv[1], "e") && !strcmp(argv[2], "--fastq-digest")) {
		int k = 3; bool d_gpu = false, no_qual = false;
		for (; k < argc; ++k) { if (!strcmp(argv[k], "--gpu") && !d_gpu) d_gpu = true; else if (!strcmp(argv[k], "--no-qual") && !no_qual) no_qual = true; else break; }
		if (argc - k != 2 && argc - k != 3) { fprintf(stderr, "usage: mcomz e --fastq-digest [--gpu] [--no-qual] IN.fastq [IN_2.fastq] OUT\n"); return 1; }
		char err[480] = ""; uint64_t n = 0;
		if (mcomh_fastq_digest_files(argv[k], argc - k == 3 ? argv[k + 1] : nullptr, 4, no_qual ? 0 : 1, d_gpu ? 0 : -1, 0, argv[argc - 1], &n, err, sizeof err)) {
			fprintf(stderr, "mcomz: no digest: %s\n", err[0] ? err : "cannot take the digest"); return 1;
		}
		printf("%llu\n", (unsigned long long)n);
		return 0;
	}
	bool gpu = false, bwt = false, names = false, fastq_names = false;
	int at = 2, qual_L = 0, fastq_L = 0;
	const char *order_path = nullptr, *mate_path = nullptr, *lossy_text = nullptr, *agree_mask = nullptr;
	long agree_Q = -1; long long mask_first = -1;
	// a canonical decimal number of at most `digits` digits, or -1
	auto number = [](const char *t, int digits) -> long long {
		if (!*t || (int)strlen(t) > digits || (t[0] == '0' && t[1])) return -1;
		long long v = 0;
		for (; *t; ++t) { if (*t < '0' || *t > '9') return -1; v = v * 10 + (*t - '0'); }
		return v;
	};
	for (; at < argc; ++at) {
		if (!strcmp(argv[at], "--gpu") && !gpu) gpu = true;
		else if (!strcmp(argv[at], "--qual") && !qual_L && at + 1 < argc) { qual_L = atoi(argv[++at]); if (qual_L < 1 || qual_L > 256) { fprintf(stderr, "mcomz: --qual takes the row length, 1 .. 256\n"); return 1; } }
		else if (!strcmp(argv[at], "--fastq-qual") && !fastq_L && at + 1 < argc) { fastq_L = atoi(argv[++at]); if (fastq_L < 1 || fastq_L > 256) { fprintf(stderr, "mcomz: --fastq-qual takes the read length, 1 .. 256\n"); return 1; } }
		else if (!strcmp(argv[at], "--order") && !order_path && at + 1 < argc) order_path = argv[++at];
		else if (!strcmp(argv[at], "--lossy") && !lossy_text && at + 1 < argc) lossy_text = argv[++at];
		else if (!strcmp(argv[at], "--agree") && !agree_mask && at + 2 < argc) {
			agree_Q = (long)number(argv[at + 1], 2); agree_mask = argv[at + 2]; at += 2;
			if (agree_Q < 0 || agree_Q > 93) { fprintf(stderr, "mcomz: --agree takes a Phred value 0 .. 93 (a decimal number without leading zeros) and the mask file\n"); return 1; }
		}
		else if (!strcmp(argv[at], "--mask-first") && mask_first < 0 && at + 1 < argc) {
			mask_first = number(argv[++at], 18);
			if (mask_first < 0) { fprintf(stderr, "mcomz: --mask-first takes a row number\n"); return 1; }
		}
		else if (!strcmp(argv[at], "--mate") && !mate_path && at + 1 < argc) mate_path = argv[++at];
		else if (!strcmp(argv[at], "--bwt") && !bwt) bwt = true;
		else if (!strcmp(argv[at], "--names") && !names) names = true;
		else if (!strcmp(argv[at], "--fastq-names") && !fastq_names) fastq_names = true;
		else break;
	}
	const bool enc = argc > 1 && !strcmp(argv[1], "e"), dec = argc > 1 && !strcmp(argv[1], "d");
	if ((!enc && !dec) || argc != at + 2 || (dec && (bwt || qual_L || fastq_L)) || (bwt && (qual_L || fastq_L)) || (qual_L && fastq_L) || (order_path && !fastq_L) || (agree_mask && !fastq_L) || (mask_first >= 0 && !agree_mask) || (lossy_text && !fastq_L && !qual_L) || (names && (dec || bwt || qual_L || fastq_L)) || (fastq_names && (dec || bwt || qual_L || fastq_L || names)) || (mate_path && enc && !names && !fastq_names)) { fprintf(stderr, "usage: mcomz e|d [--gpu] IN OUT\n       mcomz e --bwt [--gpu] IN OUT\n       mcomz e --qual L [--lossy SPEC] [--gpu] IN OUT\n       mcomz e --fastq-qual L [--order FILE] [--agree Q MASKFILE [--mask-first ROW]] [--lossy SPEC] [--gpu] IN.fastq OUT\n       mcomz e --names [--gpu] IN OUT\n       mcomz e --fastq-names [--gpu] IN.fastq OUT\n       mcomz e --names --mate TEXT1 [--gpu] IN OUT\n       mcomz e --fastq-names --mate FILE_1.fastq [--gpu] IN.fastq OUT\n       mcomz d --mate TEXT1 [--gpu] IN OUT\n       mcomz z [--gpu] IN OUT.gz\n       mcomz u [--gpu] IN.gz OUT\n"); return 1; }
	const char *in = argv[at], *out = argv[at + 1];
	const int device = gpu ? 0 : -1;
	int rc = 0;
	mcomh_qual_lossy_spec lossy; mcomh_qual_lossy_report lossy_rep = {0, 0, 0, 0};
	if (lossy_text && mcomh_qual_lossy_parse(lossy_text, &lossy)) {
		fprintf(stderr, "mcomz: --lossy takes ill8, thr:T:LO:HI (0 <= LO < T <= HI <= 93) or pblock:P (1 .. 47), decimal numbers without leading zeros; '%s' is none\n", lossy_text);
		return 1;
	}
	auto report = [&]() {
		fprintf(stderr, "lossy %s: changed %llu sum_abs %llu sum_sq %llu max_abs %llu\n", lossy_text, (unsigned long long)lossy_rep.changed, (unsigned long long)lossy_rep.sum_abs,
		        (unsigned long long)lossy_rep.sum_sq, (unsigned long long)lossy_rep.max_abs);
	};
	if (fastq_L && agree_mask) {
		char err[320] = ""; uint64_t n = 0;
		mcomh_qual_agree_report ar;
		if (mcomh_fastq_quality_member_agree(in, fastq_L, device, order_path, agree_mask, mask_first < 0 ? 0 : (uint64_t)mask_first, (uint32_t)agree_Q, lossy_text ? &lossy : nullptr, out, &n, &ar, &lossy_rep,
		                                     err, sizeof err)) { fprintf(stderr, "mcomz: %s: %s\n", in, err[0] ? err : "cannot code the qualities"); return 1; }
		fprintf(stderr, "agree %ld: mask_bits %llu changed %llu sum_abs %llu sum_sq %llu max_abs %llu\n", agree_Q, (unsigned long long)ar.mask_bits, (unsigned long long)ar.changed,
		        (unsigned long long)ar.sum_abs, (unsigned long long)ar.sum_sq, (unsigned long long)ar.max_abs);
		if (lossy_text) report();
		printf("%llu\n", (unsigned long long)n);
		return 0;
	}
	if (fastq_L && lossy_text) {
		char err[320] = ""; uint64_t n = 0;
		if (mcomh_fastq_quality_member_lossy(in, fastq_L, device, order_path, &lossy, out, &n, &lossy_rep, err, sizeof err)) { fprintf(stderr, "mcomz: %s: %s\n", in, err[0] ? err : "cannot code the qualities"); return 1; }
		report();
		printf("%llu\n", (unsigned long long)n);
		return 0;
	}
	if (fastq_L) {
		char err[320] = ""; uint64_t n = 0;
		if (order_path ? mcomh_fastq_quality_member_ordered(in, fastq_L, device, order_path, out, &n, err, sizeof err) : mcomh_fastq_quality_member(in, fastq_L, device, out, &n, err, sizeof err)) { fprintf(stderr, "mcomz: %s: %s\n", in, err[0] ? err : "cannot code the qualities"); return 1; }
		printf("%llu\n", (unsigned long long)n);
		return 0;
	}
	if (fastq_names) {
		char err[320] = ""; uint64_t n = 0;
		if (mate_path ? mcomh_fastq_name_member_mate(in, mate_path, device, out, &n, err, sizeof err) : mcomh_fastq_name_member(in, device, out, &n, err, sizeof err)) { fprintf(stderr, "mcomz: %s: %s\n", in, err[0] ? err : "cannot code the names"); return 1; }
		printf("%llu\n", (unsigned long long)n);
		return 0;
	}
	if (mate_path && dec && !has_magic(in, "MCNM")) { fprintf(stderr, "mcomz: --mate goes with a .mcn member; %s is none\n", in); return 1; }
	if (names || (dec && has_magic(in, "MCNM"))) {
		if (mate_path) rc = enc ? mcomh_name_pack_file_mate(in, mate_path, out, device) : mcomh_name_unpack_file_mate(in, mate_path, out, device);
		else rc = enc ? mcomh_name_pack_file(in, out, device) : mcomh_name_unpack_file(in, out, device);
		if (rc) fprintf(stderr, enc ? "mcomz: cannot pack %s into %s%s\n" : "mcomz: %s is not a complete, intact .mcn member, or %s cannot be written%s\n", in, out, gpu ? " (or the GPU route is not available)" : "");
		return rc ? 1 : 0;
	}
	if (qual_L || (dec && has_magic(in, "MCQV"))) {
		rc = !enc ? mcomh_qual_unpack_file(in, out, device) : lossy_text ? mcomh_qual_pack_file_lossy(in, out, qual_L, device, &lossy, &lossy_rep) : mcomh_qual_pack_file(in, out, qual_L, device);
		if (!rc && enc && lossy_text) report();
		if (rc) fprintf(stderr, enc ? "mcomz: cannot pack %s into %s%s\n" : "mcomz: %s is not a complete, intact .mcq member, or %s cannot be written%s\n", in, out, gpu ? " (or the GPU route is not available)" : "");
		return rc ? 1 : 0;
	}
	if (enc) rc = bwt ? mcomh_bwt_pack_file(in, out, device) : mcomh_entropy_pack_file(in, out, device);
	const bool bwt_in = dec && has_magic(in, "MCBW");
	if (dec) rc = bwt_in ? mcomh_bwt_unpack_file(in, out, device) : mcomh_entropy_unpack_file(in, out, device);
	if (rc) {
		fprintf(stderr, enc ? "mcomz: cannot pack %s into %s%s\n" : bwt_in ? "mcomz: %s is not a complete, intact .bwt member, or %s cannot be written%s\n"
		        : "mcomz: %s is not a complete, intact .rans member, or %s cannot be written%s\n", in, out, gpu ? " (or the GPU route is not available)" : "");
		return 1;
	}
	return 0;
}
