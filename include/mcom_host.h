/* include/mcom_host.h -- host side of the MI355X-native minicom hot path (libmcom_host.so).
 *
 * Mirrors the reference's pipeline driver for this path: the stage functions have the reference's names
 * and meaning (pre_process preprocess.c:39, kt_for_reads kthread_reads.c:247, kt_for_bucket
 * kthread_bucket.c:562, combine_cluster kthread_cb.c:570, realign_hash kthread_hash_realign.c:569,
 * updateSingle preprocess.c:243) but run their hot loops as HIP kernels through include/mcom.h.
 * The contig set lives on the device from kt_for_bucket on and is still there, complete (Stage 2's appends folded into
 * the member lists, in the reference's order), when pre_process returns; accessors, stage dumps and the stream writer
 * copy it to the host on demand.  The host keeps the loop control of the stages and orders the singleton list.
 * No CPU fallback: every stage needs the GPU.
 * Results equal the reference at one thread (-t 1, its only deterministic mode).
 */
#ifndef MCOM_HOST_H
#define MCOM_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	int k;          /* -k  0 = 31 (17 when L < 80)      minicommain.c:92-114 */
	int e;          /* -e  0 = 4                         minicommain.c:60     */
	int m;          /* -m  0 = 6                         minicommain.c:63     */
	int w;          /* -w  0 = L/2-k (3 when L < 70)     preprocess.c:89-107  */
	int cbthr;      /* -g  0 = 2e                        minicommain.c:122    */
	int max_rounds; /* -R  0 = 35                        minicommain.c:64     */
	int step;       /* -S  0 = e (5 when e > 10)         minicommain.c:130    */
	int maxthr;     /* -E  0 = L/2                       minicommain.c:140    */
	int numdict;    /* -s  0 = L/17 (L/11 when L <= 80)  kthread_hash_realign.c:153 */
	int host_threads; /* host worker threads for the consensus loops (0 = 1); results do not depend on it */
	/* The library reads NO environment variable: what changes results or the kernels used is said here.            */
	int maxsearch;      /* 0 = the reference's 500 / 2000 (preprocess.c:169-172); > 0 forces the bin cut of
	                       kthread_hash_realign.c:388 (test hook: lets a small input exercise bins above the cut)   */
	int window_scan;    /* 1 = Stage 2 with the window-driven kernel (realign_hash_search as written) instead of the
	                       read-driven one; same claims, ~50x slower: the cross-check of tests/test_gpu_realign.py   */
	int full_consensus; /* 1 = count every column of a merged contig (construct_ref2 as written) instead of only the
	                       parents' overlap; same strings (A/B switch for measurements)                             */
	int full_sketch;    /* 1 = sketch merged contigs whole instead of around the overlap; same records (A/B switch) */
	int overlap_screen; /* 1 = the first Stage-2 pass gathers the singletons' rows and screens the dictionaries on the copy stream, beside
	                       the contig index build, instead of behind it in the main stream; same result.  Measured on MI355X (100 M
	                       reads): the two kernels slow each other down by what the overlap saves (243.7 vs 245-249 ms per step), so
	                       it is off by default                                                                                 */
	int host_dump;      /* 1 = mcomh_cluster_dump, _order and _pe write their streams with the host loop (every base of every member, as the
	                       reference's print_encode does) instead of the device encoders (csrc/streams.hip); same files (A/B switch, the
	                       cross-check of tests/test_streams.py)                                                                      */
	int stream_sets;    /* number of stream sets mcomh_cluster_dump* writes (0 or 1: one).  The reference writes one set per thread -- ref.bin.T,
	                       beg_pos.bin.T, dir.bin.T, dif_char.txt.T [, ids.bin.T | ids.txt.T, peids.bin.T, file.bin.T], info.txt = "L n_threads"
	                       (kthread_dump.c:370-379) -- and its decoder takes them in parallel (decompress.c:1248-1300); here the contigs are cut
	                       into that many runs of about equal member counts.  The `minicom -t N` command line passes N (device encoders only)   */
	int stage2_join;    /* 1 = Stage 2 on one GPU as the partition-local join of round 5 (mcom_realign_join once, mcom_realign_deferred in the later
	                       passes: no index table, no dictionary screen pass) instead of the table (mcom_cindex_place + mcom_realign_pass_reads in every
	                       pass); same claims.  Measured at 100 M x 150 bp: the two take the same time, so the table stays the
	                       default; the join needs 17 GB less.  Inputs the join does not take (a dictionary bin that may exceed maxsearch, ...) go
	                       through the table by themselves                                                                                  */
	int read_batches;   /* 1 = mcomh_kt_for_reads in four batches over two streams for reads resident in HBM: the classification of a batch (bound by
	                       HBM) beside the sketch of the batch before (bound by the VALU), instead of one launch each over all reads.  Same arrays.
	                       Measured at 100 M x 150 bp, steps alternating on one box: 178.7 against 179.5 ms -- off by default                      */
} mcomh_params;

typedef struct mcomh_pipeline mcomh_pipeline;

/* reads: n rows of L upper-case ACGTN characters.  host_reads [n][L] lives in host memory and is uploaded;
 * alternatively d_reads [n][pitch] is already resident in HBM (exactly one of the two is non-NULL).      */
int  mcomh_create(mcomh_pipeline **out, int device, void *hip_stream, const uint8_t *host_reads,
                  const uint8_t *d_reads, size_t pitch, size_t n, int L, const mcomh_params *p);
/* Host-to-host form: host_reads [n][L] stays with the caller (valid until mcomh_kt_for_reads has returned) and is NOT
 * copied on the host; kt_for_reads uploads it in chunks through two device staging blocks, the copy of chunk c+1 running
 * beside classify / pack / sketch of chunk c.  Page-locked memory (hipHostMalloc, hipHostRegister) makes that overlap
 * real; pageable memory works, serialised by the runtime.  No stage dump for such a pipeline (the reads are not kept).  */
int  mcomh_create_streamed(mcomh_pipeline **out, int device, void *hip_stream, const uint8_t *host_reads, size_t n, int L,
                           const mcomh_params *p);
/* Same, from 2-bit packed rows already in HBM (include/mcom.h format, ACGT only, every read kept): the
 * entry used after the multi-GPU minimizer-bucket exchange, where a rank receives its partition packed.  */
int  mcomh_create_packed(mcomh_pipeline **out, int device, void *hip_stream, const uint64_t *d_packed, size_t n, int L,
                         const mcomh_params *p);
/* Optional, between mcomh_create_packed and mcomh_kt_for_reads: the minimizers of the packed rows are known (sketched
 * with the pipeline's k by the rank that sent them); d_x [n] hashes, d_ylow [n] position<<1 | strand.  kt_for_reads then
 * assembles the records instead of sketching the rows again.  The arrays must stay valid until kt_for_reads returns. */
/* File(s) -> pipeline (round 4; replaces bseq_open / bseq_read / bseq_read_second, bseq.c:19-66, preprocess.c:52-75).  A plain
 * four-line FASTQ file is parsed by up to 64 threads, packed by them (2 bits per base + one N flag per base: 64 bytes per read over
 * PCIe at L = 150 instead of 150) and sent straight into the pipeline's row arrays; classes, N counts and the majority-base
 * substitution are made on the device.  gzip, FASTA and multi-line records go through the sequential reader.  path2 (may be NULL):
 * the mates' file, whose reads follow those of the first.  err [err_cap]: the message of a failure.                              */
int  mcomh_create_from_fastq(mcomh_pipeline **out, int device, void *hip_stream, const char *path1, const char *path2, const mcomh_params *pp,
                             char *err, size_t err_cap);
int  mcomh_set_records(mcomh_pipeline *p, const uint64_t *d_x, const uint32_t *d_ylow);
void mcomh_destroy(mcomh_pipeline *p);
/* Device blocks of destroyed pipelines are kept for the next one of the process (a steady-state step allocates nothing); this gives
 * the free ones -- the driver's and the library's -- back to the runtime.  Both pools do so by themselves when memory runs out.    */
void mcomh_pool_trim(void);
const char *mcomh_last_error(const mcomh_pipeline *p);

int mcomh_kt_for_reads(mcomh_pipeline *p);
int mcomh_kt_for_bucket(mcomh_pipeline *p);
int mcomh_combine_cluster(mcomh_pipeline *p);
int mcomh_update_single(mcomh_pipeline *p);
/* updateSingle + realign_hash at threshold thr; *cluster_reads = reads held by contigs afterwards */
int mcomh_realign_hash(mcomh_pipeline *p, int thr, long *cluster_reads);
/* the Stage-2 loop alone (preprocess.c:197-232): passes at thr = e, e + S, ... until one adds too few reads        */
int mcomh_stage2(mcomh_pipeline *p);
/* the whole timed region of the reference: Stage 1 + Stage 2 with its loop control (preprocess.c:141-233) */
int mcomh_pre_process(mcomh_pipeline *p);
/* runs everything and writes the state after every stage in the text format of oracle/refdump.cpp */
int mcomh_dump_stages(mcomh_pipeline *p, const char *path);

/* the pre-bsc stream files of cluster_dump at one thread (kthread_dump.c:364-678),
 * single-end, not order-preserving: ref.bin.0 beg_pos.bin.0 dir.bin.0 dif_char.txt.0 info.txt single.seq
 * single_N.seq AA.txt TT.txt NN.txt, written into the existing directory `folder`.  Call after mcomh_pre_process. */
int mcomh_cluster_dump(mcomh_pipeline *p, const char *folder);
/* Inverse of those files (the reference's decompress for that mode, decompress.c:495-760): one read per line into
 * out_path, order = all-A/T/N, near-constant reads, N reads, unclustered reads, contig reads.  No GPU needed. */
int mcomh_decompress(const char *folder, const char *out_path, uint64_t *n_reads);
/* SURVEY section 8f rank 4, single-end part: the order-preserving mode (minicom -p = the reference compiled with
 * ORDER): members ordered by cmpcluster3 (kthread_cb.c:72), ids.bin.0 (kthread_dump.c:116-127), every list sorted by
 * read id with a delta-coded *.ids.bin beside it and the read count in info.txt (:377-379, :420-543); and its inverse
 * (decompress.c:109-493), which writes the reads in their original order.                                        */
int mcomh_cluster_dump_order(mcomh_pipeline *p, const char *folder);
int mcomh_decompress_order(const char *folder, const char *out_path, uint64_t *n_reads);
/* ... and the paired-end part (minicompe = the reference compiled with _PE, kthread_dump_pe.c:218-619): the pipeline
 * holds the reads of the first file as rows [0, n/2) and their mates as rows [n/2, n) (mcomh_fastq_pair_to_device);
 * besides the contig / list streams the file set carries one file bit per read and, for every read of the second
 * file, the output line of its mate (peids.bin.*, file.bin.*).  The inverse (decompress.c:780-1212) writes the first
 * file's reads to out_path1 and every mate to the same line of out_path2.                                          */
int mcomh_cluster_dump_pe(mcomh_pipeline *p, const char *folder);
int mcomh_decompress_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs);
/* The three decoders with the reads rebuilt on GPU `device` (host/mcom_decompress_gpu.cpp over csrc/decode.hip): the same files in,
 * byte-identical output files; the same archives accepted and refused.  -1 and no output file when the archive is refused, when
 * there is no such GPU (no fall back to the host decoders above: they are calls of their own) or when the rows, n x (L + 1) bytes
 * beside the stream files, do not fit the card.                                                                                  */
int mcomh_decompress_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device);
int mcomh_decompress_order_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device);
int mcomh_decompress_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device);
/* Where the last of those calls spent its time, in ms: [0] reading the files, [1] upload + indices + destinations, [2] decode (wall),
 * [3] decode kernels (device events), [4] download + write, [5] of that inside fwrite, [6] the whole call, [7] unused.              */
void mcomh_decompress_gpu_times(double *ms8);
/* Does the archive in `folder` give back exactly the reads of the FASTQ file(s)?  Answered on GPU `device` without writing a read
 * (DESIGN.md section 3.7): the file(s) go up as mcomh_fastq_to_device / mcomh_fastq_pair_to_device put them, the archive's rows are
 * rebuilt as by mcomh_decompress*_gpu (the same code up to the rows in HBM: the same archives are refused, by the same checks, before
 * anything is compared) and the two tables are compared there (mcom_verify_multiset / mcom_verify_ordered of include/mcom.h).
 * mode 0: the default archive, the reads as a multiset (the decoder returns them in another order); 1: -p, line i against line i;
 * 2: paired end (fastq2 = the mates' file, NULL in the other modes), the pairs as a multiset.
 * 0: the comparison was made, *rep says how it went (a different read COUNT is a verdict, not an error).  -1 with a message on stderr:
 * bad arguments, an archive the decoders refuse, a FASTQ that cannot be read or whose reads are not the archive's length, no such GPU
 * (there is no host route), or no room on the card for the two tables, the records and their sort.
 * What it proves: pipeline, stream writer, entropy stage and decoder -- against the reads as this project's FASTQ reader delivers them;
 * it does not prove the parser.                                                                                                      */
typedef struct {
	int identical, mode;
	uint64_t n_input, n_archive;                /* reads; mode 2: pairs */
	uint64_t missing, extra;                    /* modes 0, 2: reads (pairs) of the input that the archive does not give back, and the converse */
	uint64_t differing, first_diff;             /* mode 1: lines below min(n_input, n_archive) that differ, the first of them (~0: none) */
	uint64_t exact_runs;                        /* runs of equal hashes settled as multisets of full records (hash collisions) */
	uint64_t missing_ex[8], extra_ex[8];        /* up to 8 examples each: the smallest read (pair) numbers, ascending, from 0 */
	uint32_t n_missing_ex, n_extra_ex;
	double times_ms[8];                         /* [0] FASTQ ingest, [1] upload + indices, [2] decode, [3] compare, [4] the whole call,
	                                               [5] reading the stream files, [6] compare by device events, [7] decode kernels by device events */
} mcomh_verify_report;
int mcomh_verify_gpu(const char *folder, int mode /* 0 default, 1 order, 2 paired */, const char *fastq1, const char *fastq2 /* paired only, else NULL */,
                     int device, mcomh_verify_report *rep);
/* both files of a pair into one device matrix, second file behind the first; MCOM_E_ARG when the counts differ      */
int mcomh_fastq_pair_to_device(const char *path1, const char *path2, int device, int *L, size_t chunk_reads, uint8_t **d_reads, size_t *n,
                               char *err, size_t err_cap);

/* FASTQ / FASTA ingest (bseq_open + bseq_read, bseq.c:19-66; kseq.h), plain or gzip.
 * Every read must have the same length (bseq.c:54-57 exits otherwise; here MCOM_E_ARG).  *L == 0: taken from
 * the first read.
 *   mcomh_fastq_read      : host only, the reads into out[cap_reads][L] (MCOM_E_OVERFLOW when there are more)
 *   mcomh_fastq_to_device : the reads into HBM as [n][L] characters, parsed into two pinned chunks of chunk_reads
 *                           rows (0 = 2^20) that alternate between the parser and the copy engine; *d_reads is
 *                           what mcomh_create takes as d_reads (pitch = L); release it with mcomh_device_free.   */
int mcomh_fastq_read(const char *path, int *L, uint8_t *out, size_t cap_reads, size_t *n);
int mcomh_fastq_to_device(const char *path, int device, int *L, size_t chunk_reads, uint8_t **d_reads, size_t *n, char *err, size_t err_cap);
void mcomh_device_free(void *d_ptr);

/* ---- multi-GPU: one process per GPU, reads sharded, results identical to the single-process run ----
 * The reference is a shared-memory program (pthreads, kthread_*.c); it has no communication layer to mirror, so this
 * is new interface.  A communicator carries ONE primitive, a byte-wise all-to-all with per-peer offsets and sizes
 * (everything else -- all-gather, the sums / minima of a few counters, the MIN-reduction of the Stage-2 claim keys --
 * is built on it), over one of two transports:
 *   RCCL      ncclSend / ncclRecv between ncclGroupStart / ncclGroupEnd on the pipeline's HIP stream: every peer pair
 *             talks over its own xGMI link, no ring.  Messages are cut at 256 MiB.  librccl.so.1 is loaded on first use.
 *   callbacks the caller supplies the all-to-all for HOST buffers (MPI_Alltoallv, torch.distributed over gloo, ...);
 *             device data is staged through pinned memory.  This is what the multi-process tests use on one GPU.
 * All collective calls are synchronous and must be made by every rank in the same order.                            */
typedef struct mcomh_comm mcomh_comm;
#define MCOMH_UNIQUE_ID_BYTES 128
typedef struct {
	/* send + send_off[q] .. + send_bytes[q] goes to rank q; what rank q sent to this rank arrives at recv + recv_off[q]
	 * (recv_bytes[q] bytes; sizes agree pairwise).  Host memory.  Returns 0 on success.                              */
	int (*alltoallv)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_bytes,
	                 void *recv, const uint64_t *recv_off, const uint64_t *recv_bytes);
} mcomh_comm_ops;
/* rank 0 makes the id (ncclGetUniqueId) and hands its 128 bytes to the other ranks by any means it has */
int  mcomh_comm_unique_id(void *id128);
int  mcomh_comm_create_rccl(mcomh_comm **out, int rank, int world, const void *id128, int device);
int  mcomh_comm_create_ops(mcomh_comm **out, int rank, int world, const mcomh_comm_ops *ops, void *user);
void mcomh_comm_destroy(mcomh_comm *c);
int  mcomh_comm_rank(const mcomh_comm *c);
int  mcomh_comm_world(const mcomh_comm *c);
const char *mcomh_comm_last_error(const mcomh_comm *c);
/* the primitive and what is built on it; on_device: the buffers are HBM pointers (ordered behind hip_stream's work)  */
int  mcomh_comm_alltoallv(mcomh_comm *c, const void *send, const uint64_t *send_off, const uint64_t *send_bytes,
                          void *recv, const uint64_t *recv_off, const uint64_t *recv_bytes, int on_device, void *hip_stream);
/* rank q's part lies at buf + off[q] (bytes[q] bytes) on every rank afterwards; send = NULL: this rank's part is
 * already in place                                                                                                  */
int  mcomh_comm_allgatherv(mcomh_comm *c, const void *send, void *buf, const uint64_t *off, const uint64_t *bytes,
                           int on_device, void *hip_stream);
/* element-wise over n host values: op 0 = sum, 1 = min, 2 = max                                                     */
int  mcomh_comm_allreduce_u64(mcomh_comm *c, uint64_t *vals, size_t n, int op);
/* bytes this rank has sent to OTHER ranks so far, and the number of all-to-alls                                     */
void mcomh_comm_stats(const mcomh_comm *c, uint64_t *bytes_sent, uint64_t *calls);
/* wall seconds this rank has spent inside all-to-all calls so far (staging copies and waiting for the peers included) */
double mcomh_comm_seconds(const mcomh_comm *c);

/* The distributed pipeline: this rank holds reads [rid0, rid0 + n_local) of n_total (shards are contiguous, in rank
 * order, and cover [0, n_total); paired end: the second file's reads follow the first file's, as in mcomh_create).
 * Every stage function below works as for one GPU and must be called by all ranks; afterwards EVERY rank holds the
 * complete result (contig set, lists), identical to what mcomh_create + the same calls give on one GPU over all reads:
 *   kt_for_reads     shard-local classify / pack / sketch; packed rows, classes and N masks all-gathered
 *   kt_for_bucket    per round the minimizer records go to the owner of their bucket (bucket ranges in rank order, so
 *                    that rank-major = the reference's visiting order; rejects re-sketched with k-r move again,
 *                    kthread_bucket.c:205-212, :489-496); new contigs are all-gathered into the replicated set
 *   combine_cluster  replicated set; contig sketching and the candidate evaluation of find_next sharded by contig
 *   realign_hash     contig 17-mer index sharded by contig range, every rank probes all singletons against its part,
 *                    claim keys MIN-reduced (the claim is a minimum)
 * comm is borrowed: it must outlive the pipeline.                                                                    */
int  mcomh_create_dist(mcomh_pipeline **out, int device, void *hip_stream, mcomh_comm *comm, const uint8_t *host_reads,
                       const uint8_t *d_reads, size_t pitch, size_t n_local, uint64_t rid0, uint64_t n_total, int L,
                       const mcomh_params *p);

/* ---- the built-in entropy stage: `.rans` members (host/mcom_entropy.cpp) ----
 * The host twin of mcom_rans_encode / mcom_rans_decode (include/mcom.h): plain C++ on host buffers, no GPU, no HIP call; the same
 * bytes out for the same input and hint, the same members accepted and refused.  0 on success, -4 when cap is too small (decode:
 * *out_len = the room needed), -1 for bad arguments and for a member that is truncated, malformed or fails its CRC-32.
 *   mcomh_rans_bound     room that is enough under any model hint (hint 0 never needs more than 32 + n)
 *   mcomh_rans_estimate  the estimated coded sizes the choice compares, in the order of its preference on ties: stored, order-0 with
 *                        stride 1 / 2 / 4, order-1 with stride 1 / 2 / 4
 * File forms (what bin/mcomz runs): device = -1 the host twin, otherwise that GPU -- the file goes up and the result comes down through
 * two page-locked pieces, each copy beside the read / write of the next piece; an error, never the host twin, when there is no such
 * GPU.  No output file is left by a call that fails.  mcomh_entropy_times, ms of the last file call: [0] read (+ upload), [1] the
 * codec, [2] (download +) write, [3] the whole call, [4] raw bytes, [5] coded bytes.                                               */
uint64_t mcomh_rans_bound(uint64_t n);
int mcomh_rans_estimate(const uint8_t *in, uint64_t n, uint64_t est7[7]);
int mcomh_rans_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, int model_hint);
int mcomh_rans_decode(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len);
int mcomh_entropy_pack_file(const char *in_path, const char *out_path, int device);
int mcomh_entropy_unpack_file(const char *in_path, const char *out_path, int device);
void mcomh_entropy_times(double *ms8);

/* ---- the block-sorting coder: `.bwt` members (host/mcom_bwt.cpp) ----
 * The host twin of mcom_bwt_encode / mcom_bwt_decode (include/mcom.h): blocks of 1 MiB, Burrows-Wheeler transform with anchors every
 * 4 KiB, move-to-front, the ranks as one embedded `.rans` member -- or the plain `.rans` coding of the bytes where that is not larger.
 * Same bytes out as the device route, the same members refused.  Return values as for the rANS calls.
 *   mcomh_bwt_bound    room that is enough for n raw bytes
 *   mcomh_bwt_raw_len  the raw length a member's header states (-1: not a `.bwt` header that describes in_len bytes)
 *   mcomh_bwt_stages   the stages of the encoder for tests and tools, any of the outputs NULL: the transformed bytes (n), the index as
 *                      the member stores it (4 bytes per anchor) and the move-to-front ranks (n; needs bwt as well)
 * File forms as mcomh_entropy_pack_file / _unpack_file (mcomh_entropy_times reports them too).                                      */
uint64_t mcomh_bwt_bound(uint64_t n);
int mcomh_bwt_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len);
int mcomh_bwt_decode(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t cap, uint64_t *out_len);
int mcomh_bwt_raw_len(const uint8_t *in, uint64_t in_len, uint64_t *raw_len);
int mcomh_bwt_stages(const uint8_t *in, uint64_t n, uint8_t *bwt, uint8_t *index, uint8_t *ranks);
int mcomh_bwt_pack_file(const char *in_path, const char *out_path, int device);
int mcomh_bwt_unpack_file(const char *in_path, const char *out_path, int device);

/* ---- quality values: `.mcq` members (host/mcom_qual.cpp) ----
 * The host twin of mcom_qual_encode / mcom_qual_decode (include/mcom.h): a matrix of n_rows x L bytes, rows `pitch` >= L bytes apart,
 * under a static context model, or as an embedded `.rans` member where that is smaller.  Plain C++, no GPU; the same bytes out for the
 * same input and hint (0, 0x100 | model id 0 .. 4, 0x180 for the embedding), the same members accepted and refused.  Return values as
 * for the rANS calls; decode sets *n_rows and *L also when it returns -4 (more than cap_rows rows).
 *   mcomh_qual_bound     room that is enough under any hint (0: L outside 1 .. 256)
 *   mcomh_qual_info      n_rows and L from the first 64 bytes of a member (-1: not a `.mcq` header)
 *   mcomh_qual_estimate  the estimated sizes the choice compares, by model id 0 .. 4 (as mcomh_rans_estimate: what the tests of the
 *                        model choice and tools read)
 * mcomh_qual_estimate and the two file forms below are additions beyond the four coder calls, made on purpose on the pattern of the
 * `.rans` and `.bwt` sections above: the estimate lets a test hold the choice to the specification, the file forms are what bin/mcomz runs.
 *                                                 */
uint64_t mcomh_qual_bound(uint64_t n_rows, uint32_t L);
int mcomh_qual_info(const uint8_t *prefix, uint64_t len, uint64_t *n_rows, uint32_t *L);
int mcomh_qual_estimate(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint64_t est5[5]);
int mcomh_qual_encode(const uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, uint8_t *out, uint64_t cap, uint64_t *out_len,
                      int model_hint);
int mcomh_qual_decode(const uint8_t *in, uint64_t in_len, uint8_t *rows, uint64_t pitch, uint64_t cap_rows, uint64_t *n_rows, uint32_t *L);
/* File forms (bin/mcomz e --qual L, d): a file of n * L raw bytes <-> a `.mcq` member; device = -1 the host twin, otherwise that GPU (an
 * error, never the host twin, when there is no such GPU).  No output file is left by a call that fails.                              */
int mcomh_qual_pack_file(const char *in_path, const char *out_path, int L, int device);
int mcomh_qual_unpack_file(const char *in_path, const char *out_path, int device);

/* ---- `minicom -Q`: a -p archive that also carries the quality values, as the member qual.mcq in input order ----
 * Read names and the text of the third line are not kept: the decoders name record i `@<i+1>` and write a bare `+`.
 *   mcomh_fastq_qualities_to_device  the quality lines of a four-line FASTQ file (plain or .gz) as rows of L bytes in HBM (*d_rows,
 *                                    release with mcomh_device_free; *n records).  The text goes up through two page-locked pieces of
 *                                    piece_bytes (0 = 32 MiB; at least 4 * (2 L + 64) bytes, a smaller request is raised to that, so that a
 *                                    piece holds a few records), the unfinished record at a piece's end in front of the next piece; lines
 *                                    are found by mcom_decode_line_index, rows gathered by mcom_fastq_quality_rows.  A missing last
 *                                    newline is accepted; a record the kernel flags is an error whose message names the first one.
 *   mcomh_fastq_quality_member       FASTQ file -> the `.mcq` member file in one call (what `minicom -Q` runs, bin/mcomz e --fastq-qual L):
 *                                    on GPU `device` the two calls above and mcom_qual_encode; device = -1 the host twin of both, which
 *                                    applies the same record rules, refuses the same files and names the same first bad record.  The
 *                                    same member either way; *n = the records; no output file is left by a call that fails.
 *   mcomh_device_copy                `bytes` from one device pointer to another (for callers that hold device memory of their own, such
 *                                    as the Python mirror, and must not bind the HIP runtime a second time); 0 on success.
 *   mcomh_decompress_fastq           the host route: reads by the -p decoder, qualities by mcomh_qual_decode, four-line records.
 *   mcomh_decompress_fastq_gpu       the same bytes with reads and qualities rebuilt and the records laid out on GPU `device`.
 *   mcomh_verify_quality_gpu         qual.mcq decoded on the device against the quality lines of `fastq`, line against line
 *                                    (mcom_verify_ordered); the report's mode is 1.  Returns 0 when a comparison was made.
 * All refuse an archive that is not a -p one, that has no qual.mcq, or whose qual.mcq states another n or L than the reads; a
 * refused archive leaves no output file.                                                                                              */
int mcomh_fastq_qualities_to_device(const char *path, int device, int L, size_t piece_bytes, uint8_t **d_rows, size_t *n, char *err, size_t err_cap);
int mcomh_fastq_quality_member(const char *fastq, int L, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap);
int mcomh_device_copy(void *d_dst, const void *d_src, size_t bytes);
int mcomh_decompress_fastq(const char *folder, const char *out_path, uint64_t *n_reads);
int mcomh_decompress_fastq_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device);
int mcomh_verify_quality_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report *rep);

/* ---- `minicom -q`: a default or paired-end archive that also carries the quality values, in the archive's own order ----
 * The default and the paired-end decoder return the reads in an order of their own.  The dump knows it: with mcomh_keep_read_order it also
 * writes FOLDER/read_order.bin -- `rows` little-endian u32, the input read of the decoder's row j (paired end: of its pair j, a read of the
 * first file; the mate is read half + order[j]).  The quality rows are put into that order before they are coded, so the member needs no
 * ids beside it.  Names are not kept (the name coder codes a name against the one before it): record j is named `@<j+1>`.
 *   mcomh_keep_read_order               on != 0: from now on mcomh_cluster_dump / mcomh_cluster_dump_pe of this pipeline also write read_order.bin (by
 *                                       mcom_dump_read_order; the host_dump route writes the same bytes).  mcomh_cluster_dump_order then
 *                                       fails, and so does this call on a pipeline with a communicator.
 *   mcomh_qual_gather_rows              the host twin of mcom_qual_gather_rows (include/mcom.h): out row j = source row order[j]; *flag (cleared
 *                                       by the caller) collects MCOMH_GATHER_F_*; -1 for the arguments the device call refuses.
 *   mcomh_fastq_quality_member_ordered  mcomh_fastq_quality_member with the rows gathered through the order file first (bin/mcomz e --fastq-qual
 *                                       L --order FILE): fails with a message, and writes no member, when the file's size is no multiple of 4,
 *                                       its entry count is not the record count, or the gather raises a flag; device >= 0: also when the card
 *                                       has no room to hold the rows twice.
 *   mcomh_decompress_fastq_reordered    FOLDER with rqual.mcq -> records `@<j+1>`, read, `+`, qualities, row j the default decoder's j-th read
 *   mcomh_decompress_fastq_pe           FOLDER with rqual_1.mcq and rqual_2.mcq -> two such files, record j of one the mate of record j of the other
 *   ..._gpu                             the same bytes with reads and qualities rebuilt and the records laid out on GPU `device`
 *   mcomh_verify_records_gpu            mode 0 / 2 as mcomh_verify_gpu: the archive's (read, quality) records -- paired end: (read 1, read 2,
 *                                       quality 1, quality 2) -- against those of the FASTQ file(s) as multisets (mcom_verify_multiset_parts)
 * The decoders and the verifier refuse a -p archive, an archive of the other kind, a missing member (paired end: either one), a member of
 * another n or L than the reads and a refused member; a refused archive leaves no output file (of two, neither).                         */
#define MCOMH_GATHER_F_BOUNDS 1
#define MCOMH_GATHER_F_DUP 2
int mcomh_keep_read_order(mcomh_pipeline *p, int on);
int mcomh_qual_gather_rows(const uint8_t *rows, uint64_t n_src, uint32_t L, uint64_t pitch_in, const uint32_t *order, uint64_t n_rows, uint8_t *out,
                           uint64_t pitch_out, uint32_t *flag);
int mcomh_fastq_quality_member_ordered(const char *fastq, int L, int device, const char *order_path, const char *out_path, uint64_t *n, char *err,
                                       size_t err_cap);
int mcomh_decompress_fastq_reordered(const char *folder, const char *out_path, uint64_t *n_reads);
int mcomh_decompress_fastq_reordered_gpu(const char *folder, const char *out_path, uint64_t *n_reads, int device);
int mcomh_decompress_fastq_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs);
int mcomh_decompress_fastq_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device);
int mcomh_verify_records_gpu(const char *folder, int mode, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep);

/* ---- `minicom -b SPEC`: lossy quality values (host/mcom_qual_lossy.cpp) ----
 * A row-local, deterministic transform of the quality matrix in front of the coder: `ill8` (the eight Illumina bins), `thr:T:LO:HI`
 * (two values) and `pblock:P` (smoothing, no byte moves by more than P; NOT idempotent).  The `.mcq` format and the decoders do not
 * change; the archive says so in the plain file qual_lossy.txt (the canonical spec and a newline), and the verifiers send the FASTQ
 * file's quality rows through the same transform before they compare: the archive holds exactly T(file).
 *   mcomh_qual_lossy_parse   the canonical text (decimal numbers, no leading zeros, nothing behind it) -> spec; -1 for anything else,
 *                            a thr that is not idempotent (LO >= T or HI < T) included
 *   mcomh_qual_lossy_print   spec -> text (at most 32 bytes with the NUL); -1 for a general map or a spec the transform refuses
 *   mcomh_qual_transform     the host twin of mcom_qual_transform (include/mcom.h): the same arguments over host memory, the same bytes,
 *                            the same report, the same specs refused (-1, nothing touched)
 *   mcomh_qual_pack_file_lossy / mcomh_fastq_quality_member_lossy   mcomh_qual_pack_file and mcomh_fastq_quality_member[_ordered]
 *                            (order_path NULL: input order) with the transform between the rows and the coder: on GPU `device`
 *                            mcom_qual_transform, device = -1 the host twin; *report (may be NULL) gets the report.  A refused spec
 *                            writes nothing.  spec NULL: the calls they are named after
 *   mcomh_qual_lossy_marker  FOLDER/qual_lossy.txt: 0 = none (*spec untouched), 1 = read (spec and, when text is given, its canonical
 *                            text), -1 = there but not a canonical spec and a newline -- the verifiers refuse such an archive           */
#define MCOMH_QUAL_LOSSY_ILL8 1
#define MCOMH_QUAL_LOSSY_THR 2
#define MCOMH_QUAL_LOSSY_PBLOCK 3
#define MCOMH_QUAL_LOSSY_LUT 4
typedef struct {
	uint32_t kind;                              /* MCOMH_QUAL_LOSSY_*                                                          */
	uint32_t p[3];                              /* thr: T, LO, HI; pblock: P                                                    */
	uint8_t lut[256];                           /* MCOMH_QUAL_LOSSY_LUT: the byte map (parse fills it for the named maps too)   */
} mcomh_qual_lossy_spec;
typedef struct {
	uint64_t changed, sum_abs, sum_sq, max_abs; /* bytes that changed, sum of |d|, sum of d * d, largest |d|                    */
} mcomh_qual_lossy_report;
int mcomh_qual_lossy_parse(const char *text, mcomh_qual_lossy_spec *spec);
int mcomh_qual_lossy_print(const mcomh_qual_lossy_spec *spec, char *text, size_t cap);
int mcomh_qual_transform(uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const mcomh_qual_lossy_spec *spec, mcomh_qual_lossy_report *report);
int mcomh_qual_pack_file_lossy(const char *in_path, const char *out_path, int L, int device, const mcomh_qual_lossy_spec *spec, mcomh_qual_lossy_report *report);
int mcomh_fastq_quality_member_lossy(const char *fastq, int L, int device, const char *order_path, const mcomh_qual_lossy_spec *spec, const char *out_path,
                                     uint64_t *n, mcomh_qual_lossy_report *report, char *err, size_t err_cap);
int mcomh_qual_lossy_marker(const char *folder, mcomh_qual_lossy_spec *spec, char *text, size_t cap);

/* ---- `minicom -a Q[:C]`: consensus-guided lossy quality values (host/mcom_agree.cpp) ----
 * Every quality value of a base that agrees with its contig's consensus at a place at least C member reads cover becomes Phred Q; every
 * other value stays.  The mask is a function of the archive's own core members, so a verifier rebuilds it from the archive.  The `.mcq`
 * format and the decoders do not change; the archive says so in the plain file qual_agree.txt (`Q C` and a newline).
 *   mcomh_agree_mask       the mask of the stream files in FOLDER, written to out_path: n rows of (L + 7) / 8 bytes, row j beside row j of
 *                          the decoder's image, column i in bit i & 7 of byte i >> 3.  A folder with ids.bin.* is decoded as a -p archive,
 *                          otherwise as a default one; a paired-end default archive (file.bin.*) and a ragged one (len.bin) are refused
 *                          with a message.  What the matching decoder refuses is refused and leaves no file.  device = -1: the host
 *                          decoders' member loops; otherwise mcom_agree_coverage and mcom_agree_mask on that GPU -- the same bytes.
 *                          *bits_set = the mask bits set.  C is 1 .. 255.
 *   mcomh_qual_agree       the host twin of mcom_qual_agree (include/mcom.h): the same arguments over host memory, the same bytes, the
 *                          same report, the same arguments refused (-1, nothing touched)
 *   mcomh_fastq_quality_member_agree   mcomh_fastq_quality_member_lossy (order_path NULL: input order; spec NULL: no -b transform) with the
 *                          agreement transform behind the gather and in front of the -b transform: quality row r of the member belongs
 *                          to row first_mask_row + r of the mask file, which must hold at least that many rows of (L + 7) / 8 bytes.
 *                          On GPU `device` mcom_qual_agree, device = -1 its twin.  A call that fails writes no member.
 *   mcomh_qual_agree_marker  FOLDER/qual_agree.txt: 0 = none, 1 = read (*Q, *C), -1 = there but not `Q C` and a newline with canonical
 *                          decimal numbers in range -- the verifiers refuse such an archive
 * mcomh_verify_quality_gpu and the quality parts of mcomh_verify_order_pe_parts_gpu send the file's rows through the rebuilt mask (as far as it
 * has rows: a file of more records comes out different, not refused).  mcomh_verify_records_gpu (a `-q` archive of one file made with -a):
 * "identical" means that the file's records can be assigned one-to-one to the archive's rows so that every record has its row's read and,
 * sent through its row's mask (then through qual_lossy.txt's transform), its row's quality values; rows, quality rows and mask are made on
 * the device, the matching -- both sides sorted by read, groups of equal reads settled by augmenting paths -- is host code.  A paired-end
 * folder of the default mode that carries the marker is refused.                                                                           */
typedef struct {
	uint64_t changed, sum_abs, sum_sq, max_abs; /* as mcomh_qual_lossy_report                                                       */
	uint64_t mask_bits;                         /* mask bits set in the rows' columns                                               */
} mcomh_qual_agree_report;
int mcomh_agree_mask(const char *folder, int C, const char *out_path, int device, uint64_t *n_rows, int *L, uint64_t *bits_set);
int mcomh_qual_agree(uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const uint8_t *mask, uint64_t mask_pitch, uint64_t first_mask_row, uint32_t Q,
                     mcomh_qual_agree_report *report);
int mcomh_fastq_quality_member_agree(const char *fastq, int L, int device, const char *order_path, const char *mask_path, uint64_t first_mask_row, uint32_t Q,
                                     const mcomh_qual_lossy_spec *spec, const char *out_path, uint64_t *n, mcomh_qual_agree_report *agree_report,
                                     mcomh_qual_lossy_report *report, char *err, size_t err_cap);
int mcomh_qual_agree_marker(const char *folder, uint32_t *Q, uint32_t *C);

/* ---- BGZF output (host/mcom_bgzf.cpp) ----
 * The host twin of mcom_bgzf_encode (include/mcom.h): a plain loop over csrc/deflate_model.hpp, the same bytes as the device call.
 * Any gzip reader takes the result; the member-parallel ingest (host/mcom_fastq_gz.cpp) finds the members by their BC field.
 *   mcomh_bgzf_bound   n + 31 ceil(n / 65280) + 28
 *   mcomh_bgzf_encode  0, -1 for bad arguments, -4 when cap is too small; flags & MCOMH_BGZF_EOF appends the empty last member
 *   mcomh_bgzf_file    in_path -> out_path, closed with the empty member: device = -1 the twin, otherwise mcom_bgzf_encode on that GPU
 *                      in pieces of whole blocks (an error, never the twin, when there is no such GPU).  No output file is left by a
 *                      call that fails.                                                                                              */
#define MCOMH_BGZF_EOF 1
uint64_t mcomh_bgzf_bound(uint64_t n);
int mcomh_bgzf_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, int flags);
int mcomh_bgzf_file(const char *in_path, const char *out_path, int device);

/* ---- BGZF input inflated on the GPU (host/mcom_gzip_gpu.cpp) ----
 * The host twin of mcom_gzip_inflate (include/mcom.h): a plain loop over csrc/inflate_model.hpp, the same bytes and the same status per
 * member as the device call.  mcomh_gzip_member has the layout of mcom_gzip_member, the statuses are MCOM_GZIP_* (0 OK, 1 corrupt,
 * 2 truncated, 3 room, 4 CRC-32 or ISIZE differ).
 *   mcomh_gzip_inflate_members  the twin of the device call over a table of members: 0 when the loop ran (status[m], *bad, *first_bad
 *                               as there; status may be NULL), -1 for a table whose payloads or slots leave the buffers or whose slots
 *                               overlap or are out of order (nothing is written)
 *   mcomh_gzip_inflate          a BGZF buffer to its text: 0, -1 when the buffer is not BGZF members to its end, -4 when cap is too
 *                               small (*out_len = the room needed), otherwise the status (1 .. 4) of the first member that is not OK
 *   mcomh_gunzip_file           a BGZF file to its text (what `mcomz u` runs): device = -1 the twin, otherwise runs of whole members are
 *                               uploaded, inflated by mcom_gzip_inflate on that GPU and the text brought down (an error, never the twin,
 *                               when there is no such GPU).  -1 and no output file when a member is refused or the file is not BGZF
 *                               members (of at most 65536 bytes of text each) to its end.
 * The FASTQ passes mcomh_fastq_qualities_to_device and mcomh_fastq_names_to_device take a file whose first member carries the `BC` field
 * by this route: the members go up compressed and are inflated on the card.  The moment anything is off -- a member without `BC`, one the
 * device refuses, a walk that leaves the file, a record the kernels flag -- the file is started again from its beginning through zlib,
 * which words the error if there is one: what the two calls return does not depend on the route.                                      */
typedef struct { uint64_t in_off, in_bytes, out_off; uint32_t isize, crc; } mcomh_gzip_member;
int mcomh_gzip_inflate_members(const uint8_t *in, uint64_t in_bytes, const mcomh_gzip_member *members, uint64_t n_members,
                               uint8_t *out, uint64_t out_bytes, uint8_t *status, uint64_t *bad, uint64_t *first_bad);
int mcomh_gzip_inflate(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len);
int mcomh_gunzip_file(const char *in_path, const char *out_path, int device);

/* ---- read names and '+' lines: `.mcn` members (host/mcom_names.cpp) ----
 * The host twin of mcom_name_encode / mcom_name_decode (include/mcom.h).  The name text of n records is 2 n lines: line 1 of a record
 * without its '@', '\n', line 3 without its '+', '\n'; any byte but '\n', at most 255 bytes a line.  Names are cut into tokens and coded
 * against the record before; seven streams, each a `.bwt` member, or the `.rans` member of the text where that is smaller.  Plain C++,
 * no GPU; the same bytes out as the device route, the same members accepted and refused.  Return values as for the rANS calls.
 *   mcomh_name_bound    room that is enough for a name text of text_len bytes
 *   mcomh_name_info     n_records and text_len from the first 96 bytes of a member (-1: not a `.mcn` header)
 *   mcomh_name_encode   -1 for a text that is not 2 n complete lines or holds a line above 255 bytes: *bad_record (may be NULL) is then
 *                       the first record with such a line, ~0 otherwise
 *   mcomh_name_decode   *text_len and *n_records are set also when it returns -4 (text_len above cap)
 * File forms (bin/mcomz e --names, d): a file of name text <-> a `.mcn` member; device = -1 the host twin, otherwise that GPU (an error,
 * never the host twin, when there is no such GPU).  No output file is left by a call that fails.                                     */
uint64_t mcomh_name_bound(uint64_t text_len);
int mcomh_name_info(const uint8_t *prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len);
int mcomh_name_encode(const uint8_t *text, uint64_t text_len, uint64_t n_records, uint8_t *out, uint64_t cap, uint64_t *out_len,
                      uint64_t *bad_record);
int mcomh_name_decode(const uint8_t *in, uint64_t in_len, uint8_t *text, uint64_t cap, uint64_t *text_len, uint64_t *n_records);
int mcomh_name_pack_file(const char *in_path, const char *out_path, int device);
int mcomh_name_unpack_file(const char *in_path, const char *out_path, int device);
/* Kind 2: the name text of the second file of a pair against the first file's name text, its mate.  The host
 * twins of mcom_name_encode_mate / mcom_name_info_mate / mcom_name_decode_mate (include/mcom.h): the same bytes, the same refusals.
 *   mcomh_name_encode_mate  the member of mcomh_name_encode unless kind 2 is strictly smaller; -1 also for a mate that is not 2 n lines
 *   mcomh_name_decode_mate  kinds 0 and 1 as mcomh_name_decode (the mate is not looked at); kind 2 against `mate`, -1 for a mate of
 *                           another n_records or another crc32.  mcomh_name_decode itself refuses kind 2.
 *   mcomh_name_pack_file_mate / _unpack_file_mate   the file forms with mate_path, a file of name text (bin/mcomz e --names --mate, d --mate)
 *   mcomh_fastq_name_member_mate   mcomh_fastq_name_member for the second file of a pair: both files' name texts are gathered as there,
 *                           the member of fastq2 is coded against the names of fastq1; an error when the files differ in records      */
int mcomh_name_info_mate(const uint8_t *prefix, uint64_t len, uint64_t *n_records, uint64_t *text_len);
int mcomh_name_encode_mate(const uint8_t *text, uint64_t text_len, uint64_t n_records, const uint8_t *mate, uint64_t mate_len, uint8_t *out,
                           uint64_t cap, uint64_t *out_len, uint64_t *bad_record);
int mcomh_name_decode_mate(const uint8_t *in, uint64_t in_len, const uint8_t *mate, uint64_t mate_len, uint8_t *text, uint64_t cap,
                           uint64_t *text_len, uint64_t *n_records);
int mcomh_name_pack_file_mate(const char *in_path, const char *mate_path, const char *out_path, int device);
int mcomh_name_unpack_file_mate(const char *in_path, const char *mate_path, const char *out_path, int device);
int mcomh_fastq_name_member_mate(const char *fastq2, const char *fastq1, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap);

/* ---- `minicom -1 A_1.fastq -2 A_2.fastq -p [-Q [-N]]`: a pair kept in input order ----
 * The pipeline holds the second file's reads behind the first's, so the order-preserving dump of the 2 n rows is the archive's read part;
 * FOLDER/pe_order.txt (one line, `<n_pairs>`) marks it.  -Q adds qual_1.mcq and qual_2.mcq (n rows each), -N name_1.mcn (kind 0 or 1) and
 * name_2.mcn, coded against the first file's names where that is smaller.
 *   mcomh_cluster_dump_order_pe        mcomh_cluster_dump_order and pe_order.txt; refuses an odd number of reads
 *   mcomh_decompress_order_pe[_gpu]    rows [0, n) -> out_path1, [n, 2 n) -> out_path2, in input order
 *   mcomh_decompress_fastq_order_pe[_gpu]  four-line records: `@<j+1>` and a bare '+' in both files, or the names and '+' texts of
 *                                      name_1.mcn / name_2.mcn (name_2 decoded with the decoded name_1 text as its mate): with both, the two
 *                                      files are the two inputs byte for byte.  Host and GPU routes write the same bytes.
 *   mcomh_verify_order_pe_reads_gpu    the reads of both files line against line with the decoded rows (mode 1)
 *   mcomh_verify_quality_member_gpu / mcomh_verify_names_member_gpu   mcomh_verify_quality_gpu / mcomh_verify_names_gpu for a member of another
 *                                      name; mate_member (may be NULL): the member of the folder the name member is decoded against
 *   mcomh_verify_order_pe_parts_gpu    all checks the archive's members allow: part 0 the reads, 1 / 2 the quality lines of file 1 / 2,
 *                                      3 / 4 the names and '+' lines of file 1 / 2; present[k] says which were made
 *   mcomh_verify_order_pe_gpu          the same as one verdict
 * Refused, with neither output file left: no pe_order.txt or one that is not half the reads' number; one quality member of two; a member
 * of another n or L; name_2 without name_1 or the reverse; names without quality values (the FASTQ decoders need qual_*.mcq); any refused
 * member.  The decoders of every other archive are what they were.                                                                     */
int mcomh_cluster_dump_order_pe(mcomh_pipeline *p, const char *folder);
int mcomh_decompress_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs);
int mcomh_decompress_order_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device);
int mcomh_decompress_fastq_order_pe(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs);
int mcomh_decompress_fastq_order_pe_gpu(const char *folder, const char *out_path1, const char *out_path2, uint64_t *n_pairs, int device);
int mcomh_verify_order_pe_reads_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep);
int mcomh_verify_quality_member_gpu(const char *folder, const char *member, const char *fastq, int device, mcomh_verify_report *rep);
int mcomh_verify_names_member_gpu(const char *folder, const char *member, const char *mate_member, const char *fastq, int device, mcomh_verify_report *rep);
int mcomh_verify_order_pe_parts_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report rep[5], int present[5]);
int mcomh_verify_order_pe_gpu(const char *folder, const char *fastq1, const char *fastq2, int device, mcomh_verify_report *rep);
/* ---- `minicom -N`: a -p -Q archive that also carries read names and '+' texts, as the member name.mcn in input order ----
 *   mcomh_fastq_names_to_device  the name text of a four-line FASTQ file (plain or .gz) in HBM (*d_names, *bytes long; release with
 *                                mcomh_device_free; *n records), through two page-locked pieces of piece_bytes (0 = 32 MiB) with the
 *                                unfinished record of a piece in front of the next, as mcomh_fastq_qualities_to_device; lines by
 *                                mcom_decode_line_index, records checked and gathered by mcom_fastq_name_text.  A record without '@' or
 *                                '+', or with more than 255 bytes behind either, is an error whose message names the first one.
 *   mcomh_fastq_name_member      FASTQ file -> the `.mcn` member file (what `minicom -N` runs, bin/mcomz e --fastq-names): on GPU `device`
 *                                the call above and mcom_name_encode; device = -1 a host twin of the record rules and mcomh_name_encode.
 *                                The same member either way; *n = the records; no output file is left by a call that fails.  This is a
 *                                pass over the file of its own, beside the one that makes qual.mcq.
 *   mcomh_verify_names_gpu       name.mcn decoded on the device against the name text of `fastq`, record against record
 *                                (mcom_name_compare); the report's mode is 1.  Returns 0 when a comparison was made.
 * mcomh_decompress_fastq[_gpu] pick folder/name.mcn up by themselves: the records then carry its names and '+' texts.  They refuse a
 * name.mcn that states another n than the reads, one without qual.mcq, and a refused member; no output file is left then.             */
int mcomh_fastq_names_to_device(const char *path, int device, size_t piece_bytes, uint8_t **d_names, uint64_t *bytes, size_t *n, char *err, size_t err_cap);
int mcomh_fastq_name_member(const char *fastq, int device, const char *out_path, uint64_t *n, char *err, size_t err_cap);
int mcomh_verify_names_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report *rep);

/* ---- `minicom -p -V`: a FASTQ file whose reads differ in length (host/mcom_ragged.cpp) ----
 * L is the modal sequence length of the file (ties: the larger length).  A record whose sequence is L bases long is even: it goes to the
 * core, to qual.mcq and through the decoders' row kernels as ever.  Every other record is odd: its sequence and quality lines go to the
 * side members odd.seq and odd.qual, back to back in input order without newlines.  len.bin holds one byte per record, its length - 1;
 * its presence marks a ragged archive.  name.mcn covers all records and does not change.  A record is refused when its sequence is empty,
 * longer than 256 bases or of another length than its quality line, when a base is outside ACGTN or a quality byte outside 33 .. 126; the
 * message names the first such record, from 1.  device = -1: the plain C++ twin of every call -- the same files refused, the same first
 * bad record named, the same bytes written; otherwise that GPU (an error, never the twin, when there is no such GPU): the text goes up in
 * pieces of piece_bytes (0 = 32 MiB; at least 2304 bytes, a smaller request is raised to that), a BGZF file is inflated on the card.
 * No output file is left by a call that fails.
 *   mcomh_fastq_lengths_file           one pass over the file: len.bin to out_path, *n records, *L, *n_odd records of another length
 *   mcomh_fastq_ragged_files           line `which` (1 sequence, 3 quality) of every record: the even rows raw ([n_even][L]) to out_rows,
 *                                      the odd text to out_odd; len_path: the file the call above wrote
 *   mcomh_fastq_to_device_ragged       the even reads in HBM as [n_even][L] for mcomh_create (release with mcomh_device_free), odd.seq
 *                                      written.  The one place where the read ingest parses on the card; used under -V only.
 *   mcomh_fastq_quality_member_ragged  qual.mcq over the even rows by the unchanged quality coder, and odd.qual
 *   mcomh_fastq_emit_ragged            the twin of mcom_fastq_emit_ragged (include/mcom.h) over host memory: records first .. first +
 *                                      count - 1 into out (cap bytes; NULL: *bytes only).  -1: the tables disagree; -2: cap too small.
 * The decoders pick folder/len.bin up by themselves as they pick up name.mcn (mcomh_decompress_order[_gpu]: one read per line;
 * mcomh_decompress_fastq[_gpu]: four-line records) and refuse, leaving no output file, a folder whose parts disagree: the bytes of
 * len.bin equal to L - 1 do not number the core's reads; the other lengths do not add up to the size of odd.seq, or of odd.qual;
 * qual.mcq or name.mcn states another record count; odd.qual without qual.mcq, or the reverse.
 *   mcomh_verify_ragged_gpu            `minicom -d -c` for such an archive: the file is split again on the GPU and len.bin, the even reads,
 *                                      the even quality rows (when the archive has them) and the two odd texts are compared with what the
 *                                      archive gives back, exactly.  rep: five reports in that order (mode 1; for the odd texts `differing`
 *                                      counts bytes and first_diff is the first differing byte), present[k]: part k was compared.
 *                                      Returns 0 when the comparisons were made.                                                         */
typedef struct {                               /* mcom_ragged_src of include/mcom.h, every pointer in host memory */
	const uint8_t *reads; uint64_t read_pitch;
	const uint8_t *quals; uint64_t qual_pitch;
	uint64_t n_even;
	const uint8_t *odd_seq, *odd_qual; uint64_t odd_bytes;
	const uint64_t *slot; const uint8_t *len; uint64_t n;
	const uint8_t *names; uint64_t names_bytes; const uint64_t *rec_off;
	uint32_t L;
} mcomh_ragged_src;
int mcomh_fastq_lengths_file(const char *fastq, int device, size_t piece_bytes, const char *out_path, uint64_t *n, int *L, uint64_t *n_odd, char *err, size_t err_cap);
int mcomh_fastq_ragged_files(const char *fastq, int which, int L, int device, const char *len_path, size_t piece_bytes, const char *out_rows, const char *out_odd,
                             uint64_t *n_even, char *err, size_t err_cap);
int mcomh_fastq_to_device_ragged(const char *path, int device, int L, const char *len_path, size_t piece_bytes, uint8_t **d_reads, size_t *n_even, const char *odd_seq_path,
                                 char *err, size_t err_cap);
int mcomh_fastq_quality_member_ragged(const char *fastq, int L, int device, const char *len_path, const char *out_mcq, const char *out_odd_qual, uint64_t *n_even, char *err,
                                      size_t err_cap);
int mcomh_fastq_emit_ragged(const mcomh_ragged_src *src, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *bytes);
int mcomh_verify_ragged_gpu(const char *folder, const char *fastq, int device, mcomh_verify_report rep[5], int present[5]);

/* ---- `minicom -p -V -A`: the odd reads coded against the contigs (host/mcom_odd_align.cpp) ----
 * The plain C++ twins of the mcom_odd_* calls of include/mcom.h, every pointer in host memory: the same text T (2 bits per base in
 * (t_bases + 31) / 32 + 1 words, the last one zero), the same hits, the same member bytes, the same refusals in the same words.
 *   mcomh_odd_text_append   `bases` bases of a ref.bin image behind base `at` of T (zeroed by the caller)
 *   mcomh_odd_index_build   the sorted seed grid; release with mcomh_odd_index_free
 *   mcomh_odd_align         one hit word per record: ~0, or d << 48 | strand << 40 | p
 *   mcomh_odd_align_encode  member and residual; sizes always set, member NULL: sizes only; -2 when a capacity is too small; -1 for a hit
 *                           word that the record and T do not bear out or a text outside ACGTN
 *   mcomh_odd_align_decode  the full odd text (off[n_odd] bytes) from an untrusted member: -1 with *flags = the reasons
 *                           (mcomh_odd_align_refusal words the lowest), and out holds nothing valid
 *   mcomh_odd_align_folder  the UNGROUPED stream files of FOLDER (ref.bin.*, beg_pos.bin.*, info.txt, len.bin, odd.seq): odd.aln written and
 *                           odd.seq rewritten to the records that are not aligned -- by the device calls on GPU `device`, by the twins
 *                           with device -1, the same bytes.  No record aligned: nothing is written.  -1 with a message in err.        */
typedef struct mcomh_odd_index mcomh_odd_index;
void mcomh_odd_text_append(uint64_t *t, uint64_t at, const uint8_t *ref, uint64_t ref_bytes, uint64_t bases);
int mcomh_odd_index_build(const uint64_t *t, uint64_t t_bases, mcomh_odd_index **idx);
void mcomh_odd_index_free(mcomh_odd_index *idx);
uint64_t mcomh_odd_index_size(const mcomh_odd_index *idx);
int mcomh_odd_align(const mcomh_odd_index *idx, const uint64_t *t, uint64_t t_bases, const uint8_t *odd, const uint64_t *off, uint64_t n_odd, uint64_t *hits);
int mcomh_odd_align_encode(const uint64_t *hits, const uint8_t *odd, const uint64_t *off, uint64_t n_odd, const uint64_t *t, uint64_t t_bases, uint8_t *member,
                           uint64_t member_cap, uint64_t *member_len, uint8_t *residual, uint64_t res_cap, uint64_t *res_len);
int mcomh_odd_align_decode(const uint8_t *member, uint64_t member_len, const uint64_t *t, uint64_t t_bases, const uint8_t *residual, uint64_t res_len, const uint64_t *off,
                           uint64_t n_odd, uint8_t *out, uint32_t *flags);
const char *mcomh_odd_align_refusal(uint32_t flags);
int mcomh_odd_align_folder(const char *folder, int device, uint64_t *n_odd, uint64_t *n_aligned, uint64_t *residual_bytes, char *err, size_t err_cap);

/* ---- self-checking archives: `minicom -K` stores a digest of the input, `minicom -d` checks it (host/mcom_digest.cpp, DESIGN.md
 * section 3.18) ----
 * digest.txt is plain text, a member stored as it is: `minicom-digest 1`, `files <1|2>`, `n <records per file>`, then one line per key,
 * `<key> <16 hex digits> <16 hex digits>` (one word per seed), in the order seq.ordered.1, qual.ordered.1, name.ordered.1, the same three
 * with .2 for a pair, seq.multiset, rec.multiset.  The quality keys (qual.ordered.*, rec.multiset) are left out together when the quality
 * lines were not digested, the name keys for a file of one read per line.  The same input gives the same bytes on every route.
 *   mcomh_fastq_record_hashes  the twin of mcom_fastq_record_hashes (include/mcom.h) over host memory: the same checks, flags and words
 *   mcomh_digest_reduce        the twin of mcom_digest_reduce
 *   mcomh_fastq_digest_files   the digest of one file, or of a pair (fastq2 not NULL), as digest.txt to out_path; *n = records per file.
 *                              lines_per_record 4: four-line FASTQ records; 1: one read per line (sequence keys only).  with_qual 0: the
 *                              quality keys are left out.  device >= 0: on that GPU through the piece loop of the quality, name and length
 *                              passes (plain, .gz; a BGZF file is inflated on the card; pieces of piece_bytes, 0: 32 MiB); -1: the twins.
 *                              -1 with a message in err -- the first record that is no record, by its number from 1; two files of
 *                              different record counts; an empty file -- and no output file.
 *   mcomh_digest_print         the text of a digest: *len bytes into out (NULL: only the length; -2: cap too small)
 *   mcomh_digest_parse         the inverse; -1 with the reason in why for anything the printer does not write: an unknown key, a key
 *                              given twice or out of order, a wrong digit count, upper-case digits, a number with leading zeros, a missing
 *                              last newline, keys that are not those of a digest of that many files
 *   mcomh_digest_check         digests the decoder's output files (out2 NULL: one file; .gz included; one read per line when the
 *                              archive holds neither quality values nor names, as the decoders write it) exactly as the input was, and compares n and the keys that the archive in
 *                              `folder` can answer: with a list of ids (idsbin.tar.*, ids.bin.*, *.ids.bin: the order-preserving modes)
 *                              seq.ordered.f, qual.ordered.f when the output is FASTQ and the key is stored, name.ordered.f when there is a
 *                              name member; otherwise rec.multiset when the archive holds rqual*.mcq and the key is stored, else
 *                              seq.multiset.  0: rep says what was compared and what differed; -1: refused (no digest.txt, one that
 *                              does not parse, another number of files, an output file that is not records), the reason in rep->message. */
typedef struct {
	uint32_t files;                             /* 1 or 2                                                                          */
	uint32_t present;                           /* bit k: key k is stated (the order above, from 0)                                 */
	uint64_t n;                                 /* records per file                                                                */
	uint64_t sums[16];                          /* word 2 * key + seed                                                             */
} mcomh_digest;
typedef struct {
	int32_t identical;                          /* n and every compared key agree                                                  */
	int32_t first_diff;                         /* -1: none; -2: n; else the first key that differs                                */
	uint32_t compared, differing;               /* bit k: key k was compared / differs                                             */
	uint32_t files, reserved;
	uint64_t n_stored, n_output;
	char message[256];                          /* why the check was refused                                                       */
} mcomh_digest_report;
int mcomh_fastq_record_hashes(const uint8_t *text, uint64_t n_bytes, const uint64_t *line_start, uint64_t first_record, uint64_t n_records, int lines_per_record, uint64_t n_total,
                              uint64_t *hS, uint64_t *hQ, uint64_t *hN, uint32_t *flag);
int mcomh_digest_reduce(const uint64_t *hS1, const uint64_t *hQ1, const uint64_t *hN1, const uint64_t *hS2, const uint64_t *hQ2, const uint64_t *hN2, uint64_t n, uint64_t sums[16]);
int mcomh_fastq_digest_files(const char *fastq1, const char *fastq2, int lines_per_record, int with_qual, int device, size_t piece_bytes, const char *out_path, uint64_t *n, char *err,
                             size_t err_cap);
int mcomh_digest_print(const mcomh_digest *d, char *out, size_t cap, size_t *len);
int mcomh_digest_parse(const char *text, size_t bytes, mcomh_digest *out, char *why, size_t why_cap);
int mcomh_digest_check(const char *folder, const char *out1, const char *out2, int device, mcomh_digest_report *rep);

/* ---- a record range of a -p archive: `minicom -d -R FIRST:COUNT` ----
 * Records first .. first + count - 1 (first from 0) of what the full decode writes, and nothing else: the outputs of ranges that tile
 * [0, n), concatenated, are the full decode byte for byte, and record i keeps its identity (without name.mcn it is still `@<i+1>`).  The
 * range is clipped at the archive's end, as `head` clips; first == n or count == 0 gives an empty file and success; first > n is refused.
 * *n_written = the records written.  device >= 0: on that GPU -- phase A of the decoders unchanged, mcom_range_check_dest over every
 * source, mcom_range_decode_reads, mcom_qual_decode_rows, the names decoded whole (their CRC checked) and emitted from `first`; the
 * rows on the card are count x (L + 1) bytes, not n x (L + 1), beside the stream files, which stay whole.  A path that ends in `.gz` is
 * written as BGZF.  device == -1: the plain C++ twin, which decodes the whole table in memory and writes the slice -- the specification
 * and the cross-check, not a fast path.  Both write the same bytes and refuse the same folders.
 *   mcomh_decompress_order_range     reads, one per line
 *   mcomh_decompress_fastq_range     four-line records with qual.mcq, and name.mcn when present
 *   mcomh_decompress_order_pe_range  the same record range of BOTH files of a pair kept in input order (pe_order.txt): rows [first,
 *                                    first + count) and [half + first, half + first + count); fastq != 0: four-line records with
 *                                    qual_1.mcq / qual_2.mcq, and name_1.mcn / name_2.mcn when present
 *   mcomh_qual_decode_rows           the host twin of mcom_qual_decode_rows (include/mcom.h): rows first_row .. of a `.mcq` member, a plain
 *                                    loop over the segments they touch; the same bytes, the same members refused
 * What a range does NOT check: the CRC-32 of a quality member (it covers all rows; the touched segments' own checks stay), and, on the
 * GPU, whether a read OUTSIDE the range has its reference window inside ref.bin -- the one ground on which a range may be decoded from
 * an archive that the full decode refuses.  The syntax of every line, every size and every destination are checked as ever.
 * Refused, with a message on stderr and before a file is written: a folder that is not a -p archive (no input order to count in), a
 * `minicom -q` archive (rqual*.mcq), a ragged archive (len.bin), first > n.  -1 then, and no output file.                              */
int mcomh_decompress_order_range(const char *folder, const char *out_path, uint64_t first, uint64_t count, uint64_t *n_written, int device);
int mcomh_decompress_fastq_range(const char *folder, const char *out_path, uint64_t first, uint64_t count, uint64_t *n_written, int device);
int mcomh_decompress_order_pe_range(const char *folder, const char *out_path1, const char *out_path2, uint64_t first, uint64_t count, uint64_t *n_written, int device,
                                    int fastq);
int mcomh_qual_decode_rows(const uint8_t *in, uint64_t in_len, uint64_t first_row, uint64_t count, uint8_t *rows, uint64_t pitch, uint64_t *n_rows, uint32_t *L);

/* results */
size_t mcomh_n_contigs(const mcomh_pipeline *p);
const char *mcomh_contig_ref(const mcomh_pipeline *p, size_t i, size_t *len);   /* consensus, NOT NUL-terminated */
size_t mcomh_contig_n(const mcomh_pipeline *p, size_t i);
const uint64_t *mcomh_contig_members(const mcomh_pipeline *p, size_t i);   /* rid<<32 | offset<<1 | dir */
const uint32_t *mcomh_list(const mcomh_pipeline *p, const char *name, size_t *n); /* allA allT allN fpA fpT fpN Nfile sg */
/* The whole contig set at once, as the flat host arrays the accessors above index into: consensus strings back to back
 * (ref, string i = [ref_off[i], ref_off[i+1])), member words back to back (mem, list i = [mem_off[i], mem_off[i+1])).
 * Any of the out pointers may be NULL.  The arrays belong to the pipeline.                                          */
int mcomh_contig_set(const mcomh_pipeline *p, size_t *n_contigs, const char **ref, const uint64_t **ref_off,
                     const uint64_t **mem, const uint64_t **mem_off);
/* Digest of the result, computed where the result lives (the contig set in HBM, the lists on the host); two runs over the
 * same reads must give the same eight numbers: out = { contigs, consensus characters, members, unclustered reads (sg),
 * digest of the strings, digest of the member words, digest of the string + member offsets, digest of sg and the class
 * lists } (digests: mcom_digest sum ^ rotated xor).  Call after mcomh_pre_process.                                  */
int mcomh_result_digest(mcomh_pipeline *p, uint64_t out[8]);
/* counters: rounds merge_rounds passes windows resketch n_sg0 big_bins; timers (ms): t_reads t_bucket
 * t_combine t_realign t_gpu t_host */
double mcomh_stat(const mcomh_pipeline *p, const char *name);
/* kernel timing of the pipeline's own mcom_ctx (mcom_prof_enable / mcom_prof_read of include/mcom.h) */
int mcomh_prof_enable(mcomh_pipeline *p, int on);
int mcomh_prof_read(mcomh_pipeline *p, const char *name, double *total_ms, uint64_t *launches);
/* mcom_prof_kernels of include/mcom.h over the pipeline's contexts: "kernel<TAB>launches" lines of class `name` ("*" = all) */
int mcomh_prof_kernels(mcomh_pipeline *p, const char *name, char *buf, size_t cap, size_t *need);

#ifdef __cplusplus
}
#endif
#endif
