// minicomsg IN.fastq OUTDIR [options] -- the single-end compressor binary of the reference (minicommain.c:81-216, run by the
// script as `./minicomsg $filename $compfiles`, minicom:106), over libmcom_host.so: FASTQ -> HBM -> Stage 1 + Stage 2 ->
// the stream files of cluster_dump in OUTDIR (which must exist).  -p = the reference built with ORDER (minicom:59-62).
// -O: OUTDIR/read_order.bin as well, the input read of every row the decoder will write (`minicom -q`; not with -p).
// -V L LENFILE (with -p; `minicom -p -V`): the file's reads differ in length.  LENFILE is the len.bin that
// `mcomz e --fastq-lengths` wrote and L the modal length it printed: the reads of L bases are the archive's reads, in input order among
// themselves, and the bases of the others are written to OUTDIR/odd.seq.
#include "cli_common.hpp"
#include <string>

int main(int argc, char **argv)
{
	CliOptions o;
	int ragged_L = 0; const char *len_path = nullptr;
	for (int i = 3; i + 2 < argc; ++i)
		if (!strcmp(argv[i], "-V")) {                                          // taken out of the list: cli_parse knows options of one value
			ragged_L = atoi(argv[i + 1]); len_path = argv[i + 2];
			for (int j = i; j + 3 < argc; ++j) argv[j] = argv[j + 3];
			argc -= 3;
			break;
		}
	if (argc < 3 || !cli_parse(argc, argv, 3, o) || (len_path && (!o.order || o.keep_order || ragged_L < 1 || ragged_L > 256))) {
		fprintf(stderr, "usage: minicomsg IN.fastq OUTDIR [-k K -e E -m M -w W -s S -S STEP -E MAXTHR -g CBTHR -R ROUNDS -t THREADS -p -O -D GPU] [-p -V L LENFILE]\n"); return 1;
	}
	char err[320] = "";
	mcomh_pipeline *mp = nullptr;
	uint8_t *d_reads = nullptr;
	int rc;
	if (len_path) {
		size_t n_even = 0;
		rc = mcomh_fastq_to_device_ragged(argv[1], o.device, ragged_L, len_path, 0, &d_reads, &n_even, (std::string(argv[2]) + "/odd.seq").c_str(), err, sizeof err);
		if (!rc && (rc = mcomh_create(&mp, o.device, nullptr, nullptr, d_reads, (size_t)ragged_L, n_even, ragged_L, &o.prm))) snprintf(err, sizeof err, "no usable GPU or bad parameters");
	} else rc = mcomh_create_from_fastq(&mp, o.device, nullptr, argv[1], nullptr, &o.prm, err, sizeof err);
	if (rc) { mcomh_device_free(d_reads); fprintf(stderr, "%s: %s\n", argv[1], err[0] ? err : "cannot read the file, no usable GPU or bad parameters"); return 1; }
	const size_t n = (size_t)mcomh_stat(mp, "n"); const int L = (int)mcomh_stat(mp, "L");
	if ((rc = cli_run(mp, n, L)) || (rc = mcomh_keep_read_order(mp, o.keep_order)) || (rc = o.order ? mcomh_cluster_dump_order(mp, argv[2]) : mcomh_cluster_dump(mp, argv[2]))) { fprintf(stderr, "%s\n", mcomh_last_error(mp)); return 1; }
	mcomh_destroy(mp);
	mcomh_device_free(d_reads);
	return 0;
}
