// decompress DIR OUT pe order nthr [OUT2] -- the decoder binary of the reference (decompress.c:1225-1317, run by the
// script as `./decompress $decomp $result $pe $preserve_order $num_thr $result0`, minicom:383; pe / order are the
// words true / false).  Host only.  Unlike the reference's, which leaves per-thread part files for the script to
// concatenate (minicom:385-399), this one writes the final file(s) itself.
// decompress --gpu DIR OUT pe order nthr [OUT2]: the same with the reads rebuilt on GPU 0 (mcomh_decompress*_gpu): the same
// output files; an error, not the host decoder, when there is no GPU.
// decompress --verify DIR IN.fastq pe order nthr [IN_2.fastq]: no output file; the archive's reads are rebuilt on GPU 0 and compared there
// with the reads of the FASTQ file(s) (mcomh_verify_gpu).  Exit status 0 identical, 2 different, 1 refused or error.
// decompress --fastq [--gpu] DIR OUT.fastq: a -p -Q archive (DIR holds qual.mcq) back to four-line records `@<i+1>`, read, `+`, qualities.
// decompress --verify-quality DIR IN.fastq: qual.mcq against the quality lines of the FASTQ on GPU 0; exit status as --verify.
// decompress --verify-names DIR IN.fastq: name.mcn against the names and '+' texts of the FASTQ on GPU 0; exit status as --verify.
// decompress --fastq-reordered [--gpu] DIR OUT.fastq: a `minicom -q` archive of one file (DIR holds rqual.mcq) back to four-line records, in
// the archive's own order.  decompress --fastq-pe [--gpu] DIR OUT_1.fastq OUT_2.fastq: the paired-end one (rqual_1.mcq, rqual_2.mcq).
// decompress --verify-records DIR IN.fastq [IN_2.fastq]: the (read, quality) records -- (read 1, read 2, quality 1, quality 2) for a pair --
// of such an archive against those of the FASTQ file(s) as multisets on GPU 0; exit status as --verify.
// --fastq picks DIR/name.mcn up by itself (an archive made with -N): the records then carry the names and '+' texts.
// decompress --order-pe [--gpu] DIR OUT_1.reads OUT_2.reads: a pair kept in input order (`minicom -1 -2 -p`; DIR holds pe_order.txt): the
// first file's reads and the second's, each in its input order.  decompress --fastq-order-pe [--gpu] DIR OUT_1.fastq OUT_2.fastq: the same
// with qual_1.mcq / qual_2.mcq as four-line records, and with name_1.mcn / name_2.mcn the two input files byte for byte.
// decompress --verify-order-pe DIR IN_1.fastq IN_2.fastq: reads, quality lines and names of such an archive against the two files, each
// check the members allow, on GPU 0; exit status as --verify (1 before 2 before 0).
// decompress --verify-ragged DIR IN.fastq: an archive made with -V (DIR holds len.bin): the file is split again on
// GPU 0 and its lengths, its reads of the modal length, their quality lines and the two texts of the other reads are set against the
// archive's, part by part; exit status as --verify.  The plain decoder and --fastq pick DIR/len.bin up by themselves.
// decompress --agree-mask [--gpu] DIR C OUT: the agreement mask of `minicom -a Q[:C]` of the stream files in DIR -- a
// default-mode or a -p archive -- written to OUT; prints `n L bits_set`.  The quality verifiers pick DIR/qual_agree.txt up by themselves.
// decompress --odd-align [--gpu] DIR: `minicom -p -V -A` over the ungrouped stream files in DIR: the odd reads of
// odd.seq are searched for in the contigs of ref.bin.* (on GPU 0 with --gpu, by the host twins without: the same bytes), odd.aln is written and
// odd.seq rewritten to the reads that were not found; prints `n_odd n_aligned residual_bytes`.  The decoders pick DIR/odd.aln up by themselves.
// decompress --check-digest [--gpu] DIR OUT1 [OUT2]: an archive made with -K (DIR holds digest.txt): the output
// files are digested as the input was (on GPU 0 with --gpu, by the host twin without) and set against it, every key that the archive's
// kind can answer; one line says what was compared.  Exit status as --verify: 0 identical, 2 different, 1 refused or error.
// decompress --range FIRST COUNT ...: in front of the plain decoder of a -p archive (`[--gpu] DIR OUT false true nthr`), of --fastq and of
// --order-pe / --fastq-order-pe: records FIRST .. FIRST + COUNT - 1 (FIRST from 0, the range clipped at the archive's end) of what the mode
// writes without it, and nothing else (mcomh_decompress_*_range).  A default-mode, -q or -V archive is refused.
#include "../../../include/mcom_host.h"
#include <cstdio>
#include <cstring>

static bool g_range = false;                           // --range FIRST COUNT
static uint64_t g_first = 0, g_count = 0;

static bool decimal(const char *p, uint64_t *v)
{
	if (!*p || strlen(p) > 19) return false;
	*v = 0;
	for (; *p; ++p) { if (*p < '0' || *p > '9') return false; *v = *v * 10 + (uint64_t)(*p - '0'); }
	return true;
}

static void examples(const char *what, const uint64_t *ex, uint32_t n)
{
	if (!n) return;
	printf("  %s, for example", what);
	for (uint32_t q = 0; q < n; ++q) printf(" %llu", (unsigned long long)ex[q]);
	printf("\n");
}

// " under SPEC" for an archive made with `minicom -b SPEC` (qual_lossy.txt; the verifier has read it already, so it parses), "" otherwise
// An archive made with `minicom -a Q[:C]` (qual_agree.txt) says " under agree Q:C" in front of it.
static const char *under(const char *folder)
{
	static char text[96];
	mcomh_qual_lossy_spec sp; char spec[40];
	uint32_t Q = 0, C = 0;
	text[0] = 0;
	const bool agree = mcomh_qual_agree_marker(folder, &Q, &C) == 1;
	if (agree) snprintf(text, sizeof text, " under agree %u:%u", Q, C);
	if (mcomh_qual_lossy_marker(folder, &sp, spec, sizeof spec) == 1) snprintf(text + strlen(text), sizeof text - strlen(text), "%s under %s", agree ? " and" : "", spec);
	return text;
}

// decompress --agree-mask [--gpu] DIR C OUT: the agreement mask of the stream files in DIR as a file of n rows of
// (L + 7) / 8 bytes; prints `n L bits_set`
static int agree_mask(int argc, char **argv)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < 4) { fprintf(stderr, "usage: decompress --agree-mask [--gpu] DIR C OUT\n"); return 1; }
	int C = 0;
	{
		const char *p = argv[2];
		if (!*p || strlen(p) > 3 || (p[0] == '0')) C = -1;
		for (; C >= 0 && *p; ++p) { if (*p < '0' || *p > '9') C = -1; else C = C * 10 + (*p - '0'); }
	}
	if (C < 1 || C > 255) { fprintf(stderr, "decompress: the coverage `%s` is not a decimal number 1 .. 255\n", argv[2]); return 1; }
	uint64_t n = 0, bits = 0; int L = 0;
	if (mcomh_agree_mask(argv[1], C, argv[3], gpu ? 0 : -1, &n, &L, &bits)) {
		fprintf(stderr, "decompress: no agreement mask for %s: not a complete, consistent default-mode or -p archive%s\n", argv[1], gpu ? ", or the GPU route is not available" : "");
		return 1;
	}
	fprintf(stdout, "%llu %d %llu\n", (unsigned long long)n, L, (unsigned long long)bits);
	return 0;
}

static int check_digest(int argc, char **argv)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc != 3 && argc != 4) { fprintf(stderr, "usage: decompress --check-digest [--gpu] DIR OUT1 [OUT2]\n"); return 1; }
	mcomh_digest_report r;
	if (mcomh_digest_check(argv[1], argv[2], argc == 4 ? argv[3] : nullptr, gpu ? 0 : -1, &r)) { fprintf(stderr, "decompress: the digest of %s was not checked: %s\n", argv[1], r.message[0] ? r.message : "error"); return 1; }
	// keys: seq.ordered.1 qual.ordered.1 name.ordered.1 seq.ordered.2 qual.ordered.2 name.ordered.2 seq.multiset rec.multiset
	static const char *part[8] = {"reads", "quality lines", "names", "reads of file 2", "quality lines of file 2", "names of file 2", "reads (in any order)", "reads with their quality lines (in any order)"};
	if (r.identical) {
		const bool multi = (r.compared & 0xC0u) != 0, qual = (r.compared & 0x12u) != 0, names = (r.compared & 0x24u) != 0;
		printf("verified: %s identical to the compressed input of %llu %s\n", multi ? (r.compared & 0x80u ? "reads with their quality lines, in any order," : "reads, in any order,")
		       : qual && names ? "reads, quality lines and names" : qual ? "reads and quality lines" : names ? "reads and names" : "reads", (unsigned long long)r.n_stored, r.files == 2 ? "pairs" : "records");
		return 0;
	}
	if (r.first_diff == -2) printf("DIFFERENT: the compressed input held %llu %s, the decompressed output holds %llu\n", (unsigned long long)r.n_stored, r.files == 2 ? "pairs" : "records", (unsigned long long)r.n_output);
	else {
		printf("DIFFERENT: the decompressed output is not the compressed input: the");
		bool first = true;
		for (int k = 0; k < 8; ++k) if (r.differing >> k & 1) { printf("%s %s%s", first ? "" : ",", part[k], k < 3 && r.files == 2 ? " of file 1" : ""); first = false; }
		printf(" differ (first: %s)\n", part[r.first_diff]);
	}
	return 2;
}

static int verify(int argc, char **argv)
{
	if (argc < 6) { fprintf(stderr, "usage: decompress --verify DIR IN.fastq pe(true|false) order(true|false) nthr [IN_2.fastq]\n"); return 1; }
	const bool pe = !strcmp(argv[3], "true") || !strcmp(argv[3], "1"), order = !strcmp(argv[4], "true") || !strcmp(argv[4], "1");
	if (pe && argc < 7) { fprintf(stderr, "decompress: paired-end archives need IN_2.fastq\n"); return 1; }
	mcomh_verify_report r;
	if (mcomh_verify_gpu(argv[1], pe ? 2 : order ? 1 : 0, argv[2], pe ? argv[6] : nullptr, 0, &r)) {
		fprintf(stderr, "decompress: %s could not be verified against %s\n", argv[1], argv[2]);
		return 1;
	}
	const char *unit = pe ? "pairs" : "reads";
	if (r.identical) { printf("verified: %llu %s identical\n", (unsigned long long)r.n_input, unit); return 0; }
	printf("DIFFERENT: the FASTQ holds %llu %s, the archive %llu\n", (unsigned long long)r.n_input, unit, (unsigned long long)r.n_archive);
	if (r.mode == 1) {
		printf("  %llu lines differ", (unsigned long long)r.differing);
		if (r.differing) printf(", the first one is line %llu (from 0)", (unsigned long long)r.first_diff);
		printf("\n");
	} else {
		printf("  %llu %s of the FASTQ are missing from the archive, %llu %s of the archive are not in the FASTQ\n",
		       (unsigned long long)r.missing, unit, (unsigned long long)r.extra, unit);
		examples("missing (numbered from 0 in the FASTQ)", r.missing_ex, r.n_missing_ex);
		examples("extra (numbered from 0 in the archive's output)", r.extra_ex, r.n_extra_ex);
		if (r.exact_runs) printf("  %llu runs of equal hashes were settled record by record\n", (unsigned long long)r.exact_runs);
	}
	return 2;
}

static int verify_quality(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: decompress --verify-quality DIR IN.fastq\n"); return 1; }
	mcomh_verify_report r;
	if (mcomh_verify_quality_gpu(argv[1], argv[2], 0, &r)) { fprintf(stderr, "decompress: the qualities of %s could not be verified against %s\n", argv[1], argv[2]); return 1; }
	if (r.identical) { printf("verified: %llu quality lines identical%s\n", (unsigned long long)r.n_input, under(argv[1])); return 0; }
	printf("DIFFERENT: the FASTQ holds %llu quality lines, the archive %llu\n  %llu lines differ", (unsigned long long)r.n_input, (unsigned long long)r.n_archive, (unsigned long long)r.differing);
	if (r.differing) printf(", the first one is line %llu (from 0)", (unsigned long long)r.first_diff);
	printf("\n");
	return 2;
}

static int verify_names(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: decompress --verify-names DIR IN.fastq\n"); return 1; }
	mcomh_verify_report r;
	if (mcomh_verify_names_gpu(argv[1], argv[2], 0, &r)) { fprintf(stderr, "decompress: the names of %s could not be verified against %s\n", argv[1], argv[2]); return 1; }
	if (r.identical) { printf("verified: the names and '+' lines of %llu records identical\n", (unsigned long long)r.n_input); return 0; }
	printf("DIFFERENT: the FASTQ holds %llu records, the archive %llu\n  %llu records differ in their name or '+' line", (unsigned long long)r.n_input, (unsigned long long)r.n_archive, (unsigned long long)r.differing);
	if (r.differing) printf(", the first one is record %llu (from 0)", (unsigned long long)r.first_diff);
	printf("\n");
	return 2;
}

static int fastq(int argc, char **argv)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < 3) { fprintf(stderr, "usage: decompress --fastq [--gpu] DIR OUT.fastq\n"); return 1; }
	uint64_t n = 0;
	if (g_range ? mcomh_decompress_fastq_range(argv[1], argv[2], g_first, g_count, &n, gpu ? 0 : -1) : gpu ? mcomh_decompress_fastq_gpu(argv[1], argv[2], &n, 0) : mcomh_decompress_fastq(argv[1], argv[2], &n)) {
		fprintf(stderr, "decompress: %s is not a complete, consistent -p archive with quality values%s\n", argv[1], gpu ? ", or the GPU route is not available" : "");
		return 1;
	}
	fprintf(stdout, "%llu records\n", (unsigned long long)n);
	return 0;
}

static int fastq_reordered(int argc, char **argv, bool pe)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < (pe ? 4 : 3)) { fprintf(stderr, pe ? "usage: decompress --fastq-pe [--gpu] DIR OUT_1.fastq OUT_2.fastq\n" : "usage: decompress --fastq-reordered [--gpu] DIR OUT.fastq\n"); return 1; }
	uint64_t n = 0;
	const int rc = pe ? (gpu ? mcomh_decompress_fastq_pe_gpu(argv[1], argv[2], argv[3], &n, 0) : mcomh_decompress_fastq_pe(argv[1], argv[2], argv[3], &n))
	                  : (gpu ? mcomh_decompress_fastq_reordered_gpu(argv[1], argv[2], &n, 0) : mcomh_decompress_fastq_reordered(argv[1], argv[2], &n));
	if (rc) { fprintf(stderr, "decompress: %s is not a complete, consistent %s archive with quality values in its own order%s\n", argv[1], pe ? "paired-end" : "default-mode", gpu ? ", or the GPU route is not available" : ""); return 1; }
	fprintf(stdout, "%llu %s\n", (unsigned long long)n, pe ? "pairs" : "records");
	return 0;
}

static int verify_records(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: decompress --verify-records DIR IN.fastq [IN_2.fastq]\n"); return 1; }
	const bool pe = argc > 3;
	mcomh_verify_report r;
	if (mcomh_verify_records_gpu(argv[1], pe ? 2 : 0, argv[2], pe ? argv[3] : nullptr, 0, &r)) { fprintf(stderr, "decompress: the records of %s could not be verified against %s\n", argv[1], argv[2]); return 1; }
	const char *unit = pe ? "pairs with their quality lines" : "reads with their quality lines";
	if (r.identical) { printf("verified: %llu %s identical%s\n", (unsigned long long)r.n_input, unit, under(argv[1])); return 0; }
	printf("DIFFERENT: the FASTQ holds %llu %s, the archive %llu\n", (unsigned long long)r.n_input, unit, (unsigned long long)r.n_archive);
	printf("  %llu records of the FASTQ are missing from the archive, %llu records of the archive are not in the FASTQ\n", (unsigned long long)r.missing, (unsigned long long)r.extra);
	examples("missing (numbered from 0 in the FASTQ)", r.missing_ex, r.n_missing_ex);
	examples("extra (numbered from 0 in the archive's output)", r.extra_ex, r.n_extra_ex);
	if (r.exact_runs) printf("  %llu runs of equal hashes were settled record by record\n", (unsigned long long)r.exact_runs);
	return 2;
}

static int order_pe(int argc, char **argv, bool fastq)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < 4) { fprintf(stderr, "usage: decompress %s [--gpu] DIR OUT_1 OUT_2\n", fastq ? "--fastq-order-pe" : "--order-pe"); return 1; }
	uint64_t n = 0;
	const int rc = g_range ? mcomh_decompress_order_pe_range(argv[1], argv[2], argv[3], g_first, g_count, &n, gpu ? 0 : -1, fastq)
	             : fastq ? (gpu ? mcomh_decompress_fastq_order_pe_gpu(argv[1], argv[2], argv[3], &n, 0) : mcomh_decompress_fastq_order_pe(argv[1], argv[2], argv[3], &n))
	                     : (gpu ? mcomh_decompress_order_pe_gpu(argv[1], argv[2], argv[3], &n, 0) : mcomh_decompress_order_pe(argv[1], argv[2], argv[3], &n));
	if (rc) { fprintf(stderr, "decompress: %s is not a complete, consistent archive of a pair kept in input order%s%s\n", argv[1], fastq ? " with quality values" : "", gpu ? ", or the GPU route is not available" : ""); return 1; }
	fprintf(stdout, "%llu pairs\n", (unsigned long long)n);
	return 0;
}

static int verify_order_pe(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: decompress --verify-order-pe DIR IN_1.fastq IN_2.fastq\n"); return 1; }
	mcomh_verify_report r[5]; int present[5];
	if (mcomh_verify_order_pe_parts_gpu(argv[1], argv[2], argv[3], 0, r, present)) { fprintf(stderr, "decompress: %s could not be verified against %s and %s\n", argv[1], argv[2], argv[3]); return 1; }
	static const char *what[5] = {"reads of both files", "quality lines of file 1", "quality lines of file 2", "names and '+' lines of file 1", "names and '+' lines of file 2"};
	int rc = 0;
	for (int k = 0; k < 5; ++k) {
		if (!present[k]) continue;
		if (r[k].identical) { printf("verified: %llu %s identical%s\n", (unsigned long long)r[k].n_input, what[k], k == 1 || k == 2 ? under(argv[1]) : ""); continue; }
		rc = 2;
		printf("DIFFERENT: %s: the FASTQ holds %llu, the archive %llu\n  %llu differ", what[k], (unsigned long long)r[k].n_input, (unsigned long long)r[k].n_archive, (unsigned long long)r[k].differing);
		if (r[k].differing) printf(", the first one is %s %llu (from 0)", k >= 3 ? "record" : "line", (unsigned long long)r[k].first_diff);
		printf("\n");
	}
	return rc;
}

static int odd_align(int argc, char **argv)
{
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < 2) { fprintf(stderr, "usage: decompress --odd-align [--gpu] DIR\n"); return 1; }
	uint64_t n_odd = 0, n_aligned = 0, residual = 0;
	char err[256] = "";
	if (mcomh_odd_align_folder(argv[1], gpu ? 0 : -1, &n_odd, &n_aligned, &residual, err, sizeof err)) { fprintf(stderr, "decompress --odd-align: %s: %s\n", argv[1], err); return 1; }
	printf("%llu %llu %llu\n", (unsigned long long)n_odd, (unsigned long long)n_aligned, (unsigned long long)residual);
	return 0;
}

static int verify_ragged(int argc, char **argv)
{
	if (argc < 3) { fprintf(stderr, "usage: decompress --verify-ragged DIR IN.fastq\n"); return 1; }
	mcomh_verify_report r[5]; int present[5];
	if (mcomh_verify_ragged_gpu(argv[1], argv[2], 0, r, present)) { fprintf(stderr, "decompress: %s could not be verified against %s\n", argv[1], argv[2]); return 1; }
	static const char *what[5] = {"record lengths", "reads of the modal length", "quality lines of the reads of the modal length", "bases of the other reads", "quality values of the other reads"};
	int rc = 0;
	for (int k = 0; k < 5; ++k) {
		if (!present[k]) continue;
		if (r[k].identical) { printf("verified: %llu %s identical\n", (unsigned long long)r[k].n_input, what[k]); continue; }
		rc = 2;
		printf("DIFFERENT: %s: the FASTQ holds %llu, the archive %llu\n  %llu differ", what[k], (unsigned long long)r[k].n_input, (unsigned long long)r[k].n_archive, (unsigned long long)r[k].differing);
		if (r[k].first_diff != ~(uint64_t)0) printf(", the first one %s %llu (from 0)", k == 1 || k == 2 ? "is row" : "lies in record", (unsigned long long)r[k].first_diff);
		printf("\n");
	}
	return rc;
}

int main(int argc, char **argv)
{
	if (argc > 1 && !strcmp(argv[1], "--range")) {
		if (argc < 4 || !decimal(argv[2], &g_first) || !decimal(argv[3], &g_count)) { fprintf(stderr, "usage: decompress --range FIRST COUNT (decimal numbers, FIRST from 0) in front of a -p decode, --fastq, --order-pe or --fastq-order-pe\n"); return 1; }
		g_range = true;
		argv[3] = argv[0]; argc -= 3; argv += 3;
		const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
		const bool mode_ok = argc > 1 && (!strcmp(argv[1], "--fastq") || !strcmp(argv[1], "--order-pe") || !strcmp(argv[1], "--fastq-order-pe") || gpu || argv[1][0] != '-');
		if (!mode_ok) { fprintf(stderr, "decompress: --range goes with the plain decode of a -p archive, --fastq, --order-pe and --fastq-order-pe only\n"); return 1; }
	}
	if (argc > 1 && !strcmp(argv[1], "--check-digest")) return check_digest(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--verify-ragged")) return verify_ragged(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--agree-mask")) return agree_mask(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--odd-align")) return odd_align(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--order-pe")) return order_pe(argc - 1, argv + 1, false);
	if (argc > 1 && !strcmp(argv[1], "--fastq-order-pe")) return order_pe(argc - 1, argv + 1, true);
	if (argc > 1 && !strcmp(argv[1], "--verify-order-pe")) return verify_order_pe(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--fastq-reordered")) return fastq_reordered(argc - 1, argv + 1, false);
	if (argc > 1 && !strcmp(argv[1], "--fastq-pe")) return fastq_reordered(argc - 1, argv + 1, true);
	if (argc > 1 && !strcmp(argv[1], "--verify-records")) return verify_records(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--verify")) return verify(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--verify-quality")) return verify_quality(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--verify-names")) return verify_names(argc - 1, argv + 1);
	if (argc > 1 && !strcmp(argv[1], "--fastq")) return fastq(argc - 1, argv + 1);
	const bool gpu = argc > 1 && !strcmp(argv[1], "--gpu");
	if (gpu) { --argc; ++argv; }
	if (argc < 6) { fprintf(stderr, "usage: decompress [--gpu] DIR OUT pe(true|false) order(true|false) nthr [OUT2]\n       decompress --verify DIR IN.fastq pe order nthr [IN_2.fastq]\n"); return 1; }
	const bool pe = !strcmp(argv[3], "true") || !strcmp(argv[3], "1"), order = !strcmp(argv[4], "true") || !strcmp(argv[4], "1");
	uint64_t n = 0;
	int rc;
	if (pe) {
		if (argc < 7) { fprintf(stderr, "decompress: paired-end archives need OUT2\n"); return 1; }
		if (g_range) { fprintf(stderr, "decompress: --range needs a -p archive: a paired-end archive of the default mode keeps no input order\n"); return 1; }
		rc = gpu ? mcomh_decompress_pe_gpu(argv[1], argv[2], argv[6], &n, 0) : mcomh_decompress_pe(argv[1], argv[2], argv[6], &n);
	} else if (g_range) {
		if (!order) { fprintf(stderr, "decompress: --range needs a -p archive: without the input order there is nothing to count a range in\n"); return 1; }
		rc = mcomh_decompress_order_range(argv[1], argv[2], g_first, g_count, &n, gpu ? 0 : -1);
	} else if (gpu) rc = order ? mcomh_decompress_order_gpu(argv[1], argv[2], &n, 0) : mcomh_decompress_gpu(argv[1], argv[2], &n, 0);
	else rc = order ? mcomh_decompress_order(argv[1], argv[2], &n) : mcomh_decompress(argv[1], argv[2], &n);
	if (rc) { fprintf(stderr, "decompress: %s does not hold a complete, consistent set of stream files%s\n", argv[1], gpu ? ", or the GPU route is not available" : ""); return 1; }
	fprintf(stdout, "%llu %s\n", (unsigned long long)n, pe ? "pairs" : "reads");
	return 0;
}
