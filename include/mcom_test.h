/* mcom_test.h -- TEST HOOKS of libmcom_hip.so.  Not part of the drop-in boundary (include/mcom.h): nothing a caller of the
 * reference's functions needs is declared here.  Each hook forces a code path that real inputs reach only at sizes a unit test
 * cannot afford (a sort segment beyond the LDS, an index partition beyond the sorted placement, a consensus unit beyond the
 * bit-sliced counters) or selects between kernels that compute the same result.  Results never depend on any of them.  */
#ifndef MCOM_TEST_H
#define MCOM_TEST_H
#include "mcom.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mcom_sort_group: the size above which a segment takes the nine-pass route instead of the in-LDS sort (0 = default, at most 4096). */
int mcom_set_segment_capacity(mcom_ctx *ctx, uint32_t records);
/* mcom_cindex_build: partitions with more than `entries` entries are placed by the scattered kernel instead of
 * the sorted one (0 = all of them; negative = default).  Same index either way.                                       */
int mcom_set_index_capacity(mcom_ctx *ctx, int entries);
/* Merge consensus: a unit of 32 columns that more than `members` members reach sends its tile to the
 * wave-per-tile kernel (0 = default, the 127 the bit-sliced counters hold).  Same consensus either way.              */
int mcom_set_consensus_capacity(mcom_ctx *ctx, uint32_t members);
/* mcom_sketch_contigs has three kernels: one lane per string (windows up to 64 entries, strings below 32768 characters) with a ring of
 * 32-bit hash prefixes (k odd: ties are settled by recomputing the hashes from the string) or of 64-bit hashes, and one wave per
 * string (also the choice for 8192 strings or fewer); wave_per_string = 1 forces the last, 2 the 64-bit ring, 4 the lane per string
 * with its default ring whatever the number of strings, 0 = the default choice.  Same sketch every way.
 * mcom_set_sketch_prefix_bits (1..30; default 14: prefixes of up to 14 bits live in 16-bit ring words, wider ones in 32-bit words)
 * sets the prefix width of the first: a few bits make ties the rule (tests); wave_per_string = 3 keeps 32-bit words at any width.    */
int mcom_set_sketch_kernel(mcom_ctx *ctx, int wave_per_string);
int mcom_set_sketch_prefix_bits(mcom_ctx *ctx, int bits);
/* mcom_claim_pairs settles all rounds inside ONE launch whose workgroups meet at a grid barrier, which only works while every workgroup
 * is resident; a barrier wait that runs out raises the context's poison flag and the launch-per-round loop (two launches and a host
 * round trip per round: needs no co-residency) redoes the claiming.  route 0 = that default, 1 = the loop at once, 2 = the first barrier
 * of the one-launch kernel gives up at once (the flag trips, the loop takes over), 3 = the one-launch kernel without its tail (every round
 * by the whole grid, also when a few edges are left; by default one workgroup finishes a list of at most 16384 live edges on its own).
 * Same jobs and flags every way.
 * mcom_claim_fallbacks: how often the loop has run in this context.                                                               */
int mcom_set_claim_route(mcom_ctx *ctx, int route);
int mcom_claim_fallbacks(const mcom_ctx *ctx);
/* mcom_dicts_screen counts the singletons' (dictionary, key) pairs in hashed counters.  route 0 = the default: the counter numbers are
 * binned by counter range (a region per workgroup and bin, no global atomics) and every bin is counted in LDS; a set whose keys pile up in
 * one region (copies of one read) overflows it and goes through the global-atomics kernel instead.  1 = that kernel at once, 2 = regions of
 * a few keys, so that any input overflows (the fall-back runs).  Same answer every way.  mcom_screen_fallbacks: how often it ran.       */
int mcom_set_screen_route(mcom_ctx *ctx, int route);
int mcom_screen_fallbacks(const mcom_ctx *ctx);
/* mcom_realign_pass_reads / _tuples over a SHARE of the keys (several GPUs: geom names more than one share).  route 0 = the default: a
 * workgroup lists the (singleton, pair) tasks whose keys this share owns on a stack in LDS and a thread takes one task (k_realign_owned);
 * 1 = the kernel of the whole index with several pairs per lane, a lane dropping the pairs it does not own.  Same claims either way.  */
int mcom_set_lookup_route(mcom_ctx *ctx, int route);
/* mcom_find_next_candidates / _new / _ord test their (query, hit) pairs and list the passing ones in one of two ways.  route 0 = the
 * default: the evaluation kernel itself leaves the passing candidates in pair order (a run per workgroup, gathered behind a scan of the
 * workgroups' counts), one lane per pair; 1 = a flag per pair, a scan over the flags and a second kernel that looks the passing pairs up
 * again; 4, 8, 16 = route 0 with a group of that many lanes per pair, a lane comparing every G-th word of the overlap (measured: slower
 * than one lane at every G, csrc/contigs.hip).  Same candidates in the same order, same counts every way.                              */
int mcom_set_eval_route(mcom_ctx *ctx, int route);
/* The entropy stage (csrc/entropy.hip) has two kernels whose output never leaves the library: the histograms are only seen through the
 * 12-bit tables of the chosen model, the per-segment CRCs only after the host has joined them.  These run the very launches of
 * mcom_rans_encode / mcom_rans_decode (same grid, same aligned / byte-wise choice from the pointer, same cleared table) and hand the
 * result out.  d_in: n > 0 bytes on the device, at any address.
 * mcom_test_rans_hist: d_counts gets 4 * 256 + 7 * 65536 u64, as the encoder downloads them: the order-0 counts [i mod 4][symbol], then
 * the order-1 counts [plane][context][symbol] of the planes 0 | 1 2 | 3 4 5 6 (stride 1 | 2 | 4).
 * mcom_test_rans_seg_crc: d_crc gets one CRC-32 per segment of 2^seg_log2 bytes (8 .. 15), the last one of what is left.                */
int mcom_test_rans_hist(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint64_t *d_counts);
int mcom_test_rans_seg_crc(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint32_t seg_log2, uint32_t *d_crc);
/* The block-sorting coder (csrc/bwt.hip) hands its stages out the same way, through the launch functions mcom_bwt_encode / _decode use,
 * with the block and anchor sizes the encoder writes (2^20, 2^12).  d_in: n > 0 bytes on the device, at any address.
 * mcom_test_bwt_forward: d_bwt gets the n transformed bytes, d_idx (4-byte aligned) one u32 row per anchor in the member's order,
 * *h_rounds (may be NULL) the rounds of prefix doubling it took.
 * mcom_test_bwt_mtf: d_dst gets the move-to-front ranks of d_src's n bytes (decode != 0: the bytes of n ranks), the list starting
 * as 0 .. 255 at every block; both pointers 4-byte aligned.                                                                           */
int mcom_test_bwt_forward(mcom_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_bwt, uint32_t *d_idx, int *h_rounds);
int mcom_test_bwt_mtf(mcom_ctx *ctx, const uint8_t *d_src, uint64_t n, uint8_t *d_dst, int decode);
/* The quality coder (csrc/qual.hip) counts once, for its richest model; the counts are only seen through the tables of the chosen model.
 * mcom_test_qual_hist runs the very launches of mcom_qual_encode (alphabet pass, then the counting kernel: counters in LDS for an
 * alphabet of at most 8 values, in a global table otherwise) on n_rows > 0 rows of L bytes, `pitch` apart, at any address.  h_map gets
 * the 32 bytes of the alphabet map, *h_A the alphabet size A; d_counts (room for A * min(A, 8) * 8 * A u64; pass NULL to learn A first)
 * gets the counts [previous symbol][bin of max(s[j-2], s[j-3])][floor(8 j / L)][symbol] over dense symbols.                             */
int mcom_test_qual_hist(mcom_ctx *ctx, const uint8_t *d_rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *h_map, uint32_t *h_A,
                        uint64_t *d_counts);
/* mcom_verify_multiset keeps only the low `bits` bits of every record's hash (0 .. 63; 64 or negative = default, all of them), through
 * the same launches: with 2 or 0 bits nearly every run of equal hashes holds unequal records, so that a thousand rows walk the path
 * real data reaches once in 2^64 -- the run settled in full on the host.  Same verdict and counts at any width.                    */
int mcom_set_verify_hash_bits(mcom_ctx *ctx, int bits);
/* mcom_qual_transform's P-block kernel (csrc/qual_lossy.hip) stages tiles of whole rows in LDS, one lane per row: the rows of a tile,
 * so that a test can put its rows on both sides of a tile's edge.                                                                     */
uint32_t mcom_test_qual_pblock_tile_rows(void);
/* The one-launch prefix sums (csrc/scan.hip) and the read-back of their totals (mcom_d2h_async, csrc/api.hip), through the functions the
 * library's own callers use.  None of these changes a result.
 * mcom_test_scan_u32: the exclusive scan of n uint32 at any 4-byte aligned device addresses, d_in == d_out allowed; it does NOT wait for
 * the stream (neither does mcom_scan_u64 of mcom.h, the same for uint64 -- it only waits when the context's workspace has to grow).
 * mcom_test_scan_constants: threads of a workgroup, elements per thread of the uint32 and of the uint64 kernel (a tile = threads x
 * elements), words of the ring of totals, entries of the table that tracks them.
 * mcom_test_n_cu: the compute units the context sizes a scan's grid by (at most 2 workgroups each, at most 2048 in all).                */
int mcom_test_scan_u32(mcom_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, size_t n);
void mcom_test_scan_constants(uint32_t *threads, uint32_t *per_u32, uint32_t *per_u64, uint32_t *ring_words, uint32_t *tracked);
int mcom_test_n_cu(const mcom_ctx *ctx);
/* mcom_test_scan_script runs n_steps steps on the context's stream without waiting between them, waits at the end and returns the
 * library's error code.  d_in / d_out: two device buffers of in_bytes / out_bytes (16-byte aligned; the same buffer twice is allowed).
 * Every step is checked against these sizes, and against n_totals / copy_bytes, before the first one runs.
 *   MCOM_TEST_STEP_SCAN      scan n elements of `width` (4 | 8) bytes from element a of d_in to element b of d_out
 *   MCOM_TEST_STEP_READBACK  mcom_d2h_async of the last output element of scan step a (an earlier step) into h_totals[b]: the address
 *                            and the width that scan registered; only `width` bytes of h_totals[b] are written
 *   MCOM_TEST_STEP_LAUNCH    another kernel through MCOM_LAUNCH; n != 0: it stores the uint32 b at byte a (a multiple of 4) of d_out
 *   MCOM_TEST_STEP_COPY      mcom_d2h_async of n <= 256 bytes from byte a of d_out (width == 0) or d_in (width == 1) to byte b of h_copy
 *   MCOM_TEST_STEP_SYNC      mcom_stream_sync                                                                                        */
enum { MCOM_TEST_STEP_SCAN = 0, MCOM_TEST_STEP_READBACK = 1, MCOM_TEST_STEP_LAUNCH = 2, MCOM_TEST_STEP_COPY = 3, MCOM_TEST_STEP_SYNC = 4 };
typedef struct { uint32_t op, width; uint64_t a, b, n; } mcom_test_scan_step;
int mcom_test_scan_script(mcom_ctx *ctx, const mcom_test_scan_step *steps, size_t n_steps, void *d_in, size_t in_bytes, void *d_out, size_t out_bytes,
                          uint64_t *h_totals, size_t n_totals, uint8_t *h_copy, size_t copy_bytes);


/* ---- libmcom_host.so ---- */
struct mcomh_pipeline;
/* Multi-GPU failure protocol (minicom_amd/host/mcom_pipeline.cpp, "Failure protocol"): rank-local errors travel with a flag exchange in
 * front of every collective so that no rank is left waiting for one that has returned.  mcomh_test_inject_failure makes this rank fail
 * right before its k-th flag exchange (k = 1 ...), as if the local work in front of it had failed; mcomh_test_flag_exchanges says how
 * many a finished run made.  tests/test_gpu_distributed.py lets one rank of three fail at points spread over every stage: all three must
 * return an error, none may hang.                                                                                                   */
int  mcomh_test_inject_failure(struct mcomh_pipeline *p, long k);
long mcomh_test_flag_exchanges(const struct mcomh_pipeline *p);
/* Reads of another class than 0 reach the host as a list made on the device (mcom_special_reads): `first` entries travel with the
 * count, up to `cap` in a second copy, and beyond `cap` the class array itself is copied.  Defaults 4096 and 2^20; small values let
 * a test walk all three paths with a few dozen reads.  Before mcomh_kt_for_reads.                                              */
int  mcomh_test_special_capacity(struct mcomh_pipeline *p, uint32_t first, uint32_t cap);
/* A gzip file of several members is inflated and parsed by all cores (host/mcom_fastq_gz.cpp); whatever that route does not take goes to
 * the sequential reader, with the same rows.  Work items (groups of members) of the last file the parallel route read to its end, 0 when
 * the last file went to the sequential reader: lets a test tell which of the two it has checked.                                    */
long mcomh_test_gz_items(void);
/* The member-parallel route decodes with its own DEFLATE decoder (host/mcom_inflate.cpp), not zlib: one gzip member at in[0 .. in_n) into
 * out[0 .. out_cap).  0 = decoded (*in_used bytes were the member, *out_n bytes came out, CRC-32 and ISIZE checked), 1 = out is too
 * small, < 0 = truncated (-1) / not a valid member (-2).  For tests that hold it against zlib.                                        */
int  mcomh_test_gunzip(const uint8_t *in, size_t in_n, uint8_t *out, size_t out_cap, size_t *in_used, size_t *out_n);
/* The GPU decoders (host/mcom_decompress_gpu.cpp) bring their output down in pieces of 64 MiB; with a `.gz` path the text below one BGZF
 * block at a piece's end is carried in front of the next piece.  The piece size in bytes (0 = the default, otherwise at least 4096) for the
 * calls that follow: a test of a few thousand records then crosses many pieces.  The files written never depend on it.  A piece has to
 * hold one record: the FASTQ tails refuse an archive whose records (2 L + 17 bytes, a name in place of the number up to 512 more) do not
 * fit, so the smallest size serves reads up to about 1700 bases.                                                                     */
int  mcomh_test_decoder_piece_bytes(size_t bytes);
/* The FASTQ passes over a BGZF file inflate its members on the card (host/mcom_gzip_gpu.cpp): members inflated on the device by the last
 * call of mcomh_fastq_qualities_to_device or mcomh_fastq_names_to_device, 0 when zlib's reader took the file.                         */
long mcomh_test_gz_device_members(void);

#ifdef __cplusplus
}
#endif
#endif
