// mcomz e|d [--gpu] [--bwt] IN OUT -- the built-in entropy stage as a program: it stands where the reference's script runs `bsc e IN OUT`
// and `bsc d IN OUT` (minicom:115, :346).  e: IN -> a `.rans` member, with --bwt a `.bwt` member (the block-sorting coder, DESIGN.md
// section 3.8); d: the way back, the kind of member taken from its first four bytes.  Host twin by default, GPU 0 with --gpu (an error,
// not the host twin, when there is none).  Exit status 1 and no output file when IN cannot be read, is not a complete, intact member, or
// OUT cannot be written.
#include "../../../include/mcom_host.h"
#include <cstdio>
#include <cstring>

static bool is_bwt_member(const char *path)
{
	char magic[4] = {0, 0, 0, 0};
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	const bool got = fread(magic, 1, 4, f) == 4;
	fclose(f);
	return got && !memcmp(magic, "MCBW", 4);
}

int main(int argc, char **argv)
{
	bool gpu = false, bwt = false;
	int at = 2;
	for (; at < argc; ++at) {
		if (!strcmp(argv[at], "--gpu") && !gpu) gpu = true;
		else if (!strcmp(argv[at], "--bwt") && !bwt) bwt = true;
		else break;
	}
	const bool enc = argc > 1 && !strcmp(argv[1], "e"), dec = argc > 1 && !strcmp(argv[1], "d");
	if ((!enc && !dec) || argc != at + 2 || (dec && bwt)) { fprintf(stderr, "usage: mcomz e|d [--gpu] IN OUT\n       mcomz e --bwt [--gpu] IN OUT\n"); return 1; }
	const char *in = argv[at], *out = argv[at + 1];
	const int device = gpu ? 0 : -1;
	int rc = 0;
	if (enc) rc = bwt ? mcomh_bwt_pack_file(in, out, device) : mcomh_entropy_pack_file(in, out, device);
	const bool bwt_in = dec && is_bwt_member(in);
	if (dec) rc = bwt_in ? mcomh_bwt_unpack_file(in, out, device) : mcomh_entropy_unpack_file(in, out, device);
	if (rc) {
		fprintf(stderr, enc ? "mcomz: cannot pack %s into %s%s\n" : bwt_in ? "mcomz: %s is not a complete, intact .bwt member, or %s cannot be written%s\n"
		        : "mcomz: %s is not a complete, intact .rans member, or %s cannot be written%s\n", in, out, gpu ? " (or the GPU route is not available)" : "");
		return 1;
	}
	return 0;
}
