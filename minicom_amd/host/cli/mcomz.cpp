// mcomz e|d [--gpu] IN OUT -- the built-in entropy stage as a program: it stands where the reference's script runs `bsc e IN OUT` and
// `bsc d IN OUT` (minicom:115, :346).  e: IN -> a `.rans` member; d: the way back.  Host twin by default, GPU 0 with --gpu (an error,
// not the host twin, when there is none).  Exit status 1 and no output file when IN cannot be read, is not a complete, intact member, or
// OUT cannot be written.
#include "../../../include/mcom_host.h"
#include <cstdio>
#include <cstring>

int main(int argc, char **argv)
{
	const bool gpu = argc > 2 && !strcmp(argv[2], "--gpu");
	const bool enc = argc > 1 && !strcmp(argv[1], "e"), dec = argc > 1 && !strcmp(argv[1], "d");
	if ((!enc && !dec) || argc != (gpu ? 5 : 4)) { fprintf(stderr, "usage: mcomz e|d [--gpu] IN OUT\n"); return 1; }
	const char *in = argv[gpu ? 3 : 2], *out = argv[gpu ? 4 : 3];
	const int rc = enc ? mcomh_entropy_pack_file(in, out, gpu ? 0 : -1) : mcomh_entropy_unpack_file(in, out, gpu ? 0 : -1);
	if (rc) {
		fprintf(stderr, enc ? "mcomz: cannot pack %s into %s%s\n" : "mcomz: %s is not a complete, intact .rans member, or %s cannot be written%s\n", in, out,
		        gpu ? " (or the GPU route is not available)" : "");
		return 1;
	}
	return 0;
}
