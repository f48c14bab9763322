/*
 * urmapx.h -- C ABI of the MI355X-native urmap mapping path (liburmapx.so).
 *
 * The reference (rcedgar/urmap) has no plugin / FFI layer: the per-read path is compiled
 * into its one executable.  The seam it uses internally is
 *     State1::SetMethod / State1::SetUFI / State1::Search / State1::Output1   (map.cpp:11-25)
 *     UFIndex::FromFile                                                        (ufindexio.cpp:51-115)
 * and this header is the batch form of exactly that seam: plain pointers and sizes, no
 * C++ or torch types, error codes instead of Die()/exit (myutils.cpp:915).
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * All functions return 0 on success or a negative URMAPX_E_* code.  Nothing in this
 * library has a CPU fallback: without a HIP device every compute entry point returns
 * URMAPX_E_NODEVICE.
 */
#ifndef URMAPX_H
#define URMAPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URMAPX_OK 0
#define URMAPX_E_IO (-1)          /* cannot open / short read */
#define URMAPX_E_FORMAT (-2)      /* bad .ufi magic or header */
#define URMAPX_E_NOMEM (-3)       /* host or device allocation failed */
#define URMAPX_E_NODEVICE (-4)    /* no usable HIP device / HIP runtime error */
#define URMAPX_E_ARG (-5)         /* invalid argument */
#define URMAPX_E_UNSUPPORTED (-6) /* input outside the device path's domain (see status bits) */

/* per-read status bits (urmapx_result.status); non-zero => that read's result is not valid */
/* Single-end: a read the fast kernels flag is mapped again by the general kernel (lists in global memory), so these
 * remain only beyond ITS limits: 65536 live hits, 65536..262144 HSPs, a batch's path arena full, a flank window clipped
 * by the end of the sequence store with a band beyond 1100 columns, a read shorter than the word length (the reference
 * underflows there) or longer than URMAPX_MAX_QL_SLOW (where the reference stops with an assertion).  Paired-end: none either since
 * round 4 (the general pair kernel, kernels_pe_slow.hip), except mates beyond the reference's own byte-sized pending positions. */
#define URMAPX_ST_HIT_OVERFLOW 0x01 /* more live hits than the device lists hold */
#define URMAPX_ST_HSP_OVERFLOW 0x02 /* more HSPs than the device lists hold */
#define URMAPX_ST_PATH_OVERFLOW 0x04 /* alignment path longer than the path storage */
#define URMAPX_ST_BAND_TOO_WIDE 0x08 /* DP problem larger than the wide-band scratch */
#define URMAPX_ST_BAD_LENGTH 0x10    /* read shorter than the word length or longer than the kernels take */

#define URMAPX_MAX_QL 1024    /* single-end reads the fast kernels take.  Paired-end mates: at most 320 bases AND at most 256 k-mer starts (QL - W + 1 <= 256: the reference keeps pending seed positions in a byte, state1.h:86-87), i.e. 279 bases at the default word length 24 */
#define URMAPX_MAX_QL_SLOW 30836 /* single-end reads the general kernel takes (lists in global memory): the reference's own limit -- its per-read scratch is a 1 MB bump allocator (state1.h:113,208-213) that a read of 30 837 bases overruns ("assert failed: m_AllocBuffOffset <= m_AllocBuffSize", measured with the reference binary) */
#define URMAPX_MAX_PATH_OPS 96

typedef struct urmapx_index urmapx_index;
typedef struct urmapx_ctx urmapx_ctx;

/* State1::SetMethod constants (state1.cpp:147-183). */
typedef struct urmapx_params {
	int32_t mismatch_score;
	int32_t gap_open_score;
	int32_t gap_ext_score;
	int32_t min_hsp_score_pct;
	int32_t term_hsp_score_pct_phase3;
	int32_t xdrop;
	int32_t max_penalty;
	int32_t xphase1, xphase3, xphase4;
	uint32_t band_radius;
} urmapx_params;

/* method 6 = urmap -map default, 7 = -veryfast (state1.cpp:152-179) */
int urmapx_params_for_method(unsigned method, urmapx_params *out);

/* One read's outcome of State1::Search (search1.cpp:7-24) incl. SetMappedPos (state1.cpp:129-145). */
typedef struct urmapx_result {
	uint32_t dbpos;     /* top hit start in the concatenated sequence; UINT32_MAX = unmapped */
	uint32_t seq_index; /* sequence directory index, UINT32_MAX if unmapped */
	uint32_t coord;     /* 0-based position in that sequence */
	int16_t score;      /* m_BestScore */
	int16_t second;     /* m_SecondBestScore */
	uint8_t mapq;       /* m_Mapq */
	uint8_t plus;       /* 1 = read maps as given, 0 = reverse complement */
	uint8_t exit_phase; /* 1..6: phase of Search_Lo (search1m6.cpp:35-277) that returned */
	uint8_t status;     /* URMAPX_ST_* bits */
	uint16_t hit_count; /* m_HitCount */
	uint16_t path_nops; /* 0 => ungapped ("<QL>M"); else run count in the path arena */
	uint32_t path_off;  /* first run of this read in the path arena */
} urmapx_result;

/* Path arena entry: (len << 2) | code; code 0 = M, 1 = D (query base vs gap), 2 = I (target base vs gap),
 * the reference's own path alphabet (pathinfo.h); CIGAR swaps D and I (cigar.cpp:22-25). */
typedef uint16_t urmapx_path_op;

/* ---- index: UFIndex::FromFile (ufindexio.cpp:51-115) + the device-load path ---- */
int urmapx_index_open(const char *ufi_path, urmapx_index **out);
/* The same file straight into the HBM of `device` (round 5): the header is parsed on the host, the slot table and the sequence store
 * stream from the file through page-locked buffers read by several threads, and the resident layouts are built there; no host copy
 * of the arrays is kept (urmapx_index_replicate copies device to device from such an index).  What `urmap -map / -map2` loads with. */
int urmapx_index_open_device(const char *ufi_path, int device, urmapx_index **out);
/* Wrap caller-owned HOST arrays (no copy; must outlive the index).  labels = seq_count NUL-terminated strings. */
int urmapx_index_wrap_host(uint32_t word_length, uint32_t max_ix, uint64_t slot_count, const uint8_t *blob,
                           const uint8_t *seqdata, uint32_t seqdata_size, uint32_t seq_count,
                           const uint32_t *seq_lengths, const uint32_t *offsets, const char *labels,
                           urmapx_index **out);
/* Adopt caller-owned DEVICE arrays on `device` (index already resident in HBM, e.g. built there).
 * d_blob must have >= 5*slot_count+8 bytes, d_seqdata >= seqdata_size+4096 bytes with the tail zeroed. */
int urmapx_index_wrap_device(int device, uint32_t word_length, uint32_t max_ix, uint64_t slot_count,
                             const void *d_blob, const void *d_seqdata, uint32_t seqdata_size, uint32_t seq_count,
                             const uint32_t *seq_lengths, const uint32_t *offsets, const char *labels,
                             urmapx_index **out);
/* Copy slot table + sequence to HBM of `device` (once per GPU); no-op if already resident there. */
int urmapx_index_upload(urmapx_index *, int device);
/* A second, third... replica of an index that has its host arrays (opened or wrapped) in the HBM of another device:
 * one replica per GPU, reads sharded across them, no exchange between devices (the reference's threads share one
 * UFIndex, map.cpp:43-61).  The new object borrows src's host arrays: close it before src. */
int urmapx_index_replicate(const urmapx_index *src, int device, urmapx_index **out);
void urmapx_index_close(urmapx_index *);

/* bytes of GetRow_Blob's rows laid out beside the resident slot table (chain_rows.hip); 0 if they were not built */
uint64_t urmapx_index_chain_row_bytes(const urmapx_index *);
/* UFIndex::Validate / cmd_ufi_validate (ufindex.cpp:611-658, ufistats.cpp:141-147) as one pass over the RESIDENT table (the
 * index must have been uploaded or wrapped on a device): every slot whose tally says "mine" heads a row; the row is collected
 * link by link as GetRow_Validate does (ufindex.cpp:834-881: head "mine", later links "other", the middle slot of a long link
 * TALLY_NEXT_LONG_OTHER, at most MaxIx entries), every position must lie inside the sequence store and the word that starts
 * there must hash back to the head slot (the reference dies with "WordToSlot != Slot").  Beyond the reference's test, every
 * slot that is not free must lie on exactly one head's chain (reached == used).  Returns URMAPX_OK for a valid table,
 * URMAPX_E_FORMAT if any check failed (the report says which), URMAPX_E_ARG if the index is not resident. */
typedef struct urmapx_validate_report {
	uint64_t slots;          /* slots of the table */
	uint64_t heads;          /* slots that head a row (tally "mine") */
	uint64_t positions;      /* stored positions re-hashed */
	uint64_t used;           /* slots that are not TALLY_FREE */
	uint64_t reached;        /* slots the walks passed through (chain links and the middle slots of long links) */
	uint64_t bad_hash;       /* positions whose word does not hash to the head slot */
	uint64_t bad_pos;        /* positions outside the sequence store */
	uint64_t bad_link;       /* mine / other bits, long-link middle slots or steps that break the chain rules */
	uint64_t bad_len;        /* rows longer than MaxIx */
	uint64_t first_bad_slot; /* lowest head slot with a failure; UINT64_MAX: none */
	double seconds;          /* the pass on the device */
} urmapx_validate_report;
int urmapx_index_validate(const urmapx_index *, urmapx_validate_report *out);
/* The index statistics of -ufi_stats (UFIndex::LogStats, ufistats.cpp:5-124) as two device passes over the RESIDENT table
 * (ufi_stats.hip).  The sequence passes look at [0, SeqDataSize - 1), as the reference's do (ufindexio.cpp:70-71).  Counters are
 * 64 bit where the reference's are 32-bit `unsigned`: the two agree below 2^32.  Returns URMAPX_OK; URMAPX_E_ARG if the index is not
 * resident; URMAPX_E_UNSUPPORTED for a word length over 32; URMAPX_E_FORMAT if a row is damaged (K >= 256, or a position at or past
 * the sequence store where the reference would compare its bytes; the reference asserts), with bad_rows and first_bad_slot set and
 * the collision count leaving those rows out.  Two byte arrays of slot_count bytes each live on the device for the call. */
typedef struct urmapx_ufi_stats {
	uint64_t word_length, max_ix, seqdata_size, slots;
	uint64_t indexed;     /* complete words whose start position is in their slot's row (CountIndexedWords) */
	uint64_t not_indexed; /* complete words whose start is not */
	uint64_t wildcard;    /* positions where no complete word ends */
	uint64_t indexed2;    /* sum over every slot of its row length (GetCollisionCount) */
	uint64_t free;        /* tally classes over every slot */
	uint64_t collision;   /* row entries k >= 1 whose W raw bytes differ from entry 0's */
	uint64_t single_both, single_plus, end, mine, other;
	uint64_t trunc, trunc2; /* slots whose row the MaxIx cap cut: sum of their plus counts, their number */
	uint64_t long_mine, long_other;
	uint64_t total;       /* sum of the (saturated) plus counts */
	uint64_t bad_rows;    /* damaged rows (see above) */
	uint64_t first_bad_slot; /* lowest damaged head slot; UINT64_MAX: none */
	uint64_t count_hist[256]; /* slots whose plus count is n */
	uint64_t trunc_hist[256]; /* truncated slots whose plus count is n */
	double position_seconds;  /* the pass over the sequence on the device */
	double slot_seconds;      /* the pass over the slots */
} urmapx_ufi_stats;
int urmapx_index_stats(const urmapx_index *, urmapx_ufi_stats *out);
/* UFIndex::CountSlots (minus = 0; the bytes -ufi_counts writes) or CountSlots_Minus (minus != 0) of the resident table into
 * host_out: one byte per slot, the number of words that hash there saturated at 255.  n must equal the slot count (URMAPX_E_ARG). */
int urmapx_index_slot_counts(const urmapx_index *, int minus, uint8_t *host_out, uint64_t n);
/* -ufi_info (ufistats.cpp:148-175): the 24-byte header of a .ufi file only, on the host.  URMAPX_E_IO if it cannot be read,
 * URMAPX_E_FORMAT if the magic is wrong.  Any output pointer may be NULL. */
int urmapx_ufi_info(const char *path, uint32_t *word_length, uint32_t *max_ix, uint32_t *seqdata_size, uint64_t *slot_count);
/* Which bytes is this?  Checksum of a device-resident array: the sum, modulo 2^64, over its little-endian 64-bit words w_i
 * (i = 0, 1, ...; the last word zero-padded) of murmur64(w_i + (i + 1) * 0x9E3779B97F4A7C15) with the reference's murmur64
 * (ufindex.h:50-58).  d_ptr must be 8-byte aligned.  A sum, so the same array gives the same value on every device and in the
 * numpy restatement of tests/oracle_lib.py.  urmapx_index_checksum: out[0] the resident slot table (5 * slot_count bytes, the
 * .ufi file's m_Blob), out[1] the sequence store (seqdata_size bytes, m_SeqData) -- bench.py prints both so that a run says which
 * genome and which table it mapped against (the reference has no counterpart; its -ufi_validate checks consistency, not identity). */
int urmapx_checksum_device(int device, const void *d_ptr, uint64_t nbytes, uint64_t *out);
int urmapx_index_checksum(const urmapx_index *, uint64_t out[2]);
/* the same over the layouts DERIVED from the table at upload: out[0] slot16 (16 * slot_count bytes), out[1] the chain rows (4 bytes per
 * position); 0 for a layout that was not built.  Two uploads of one table must agree, whichever way the layouts were built. */
int urmapx_index_layout_checksum(const urmapx_index *, uint64_t out[2]);
uint32_t urmapx_index_word_length(const urmapx_index *);
uint32_t urmapx_index_max_ix(const urmapx_index *);
uint64_t urmapx_index_slot_count(const urmapx_index *);
uint32_t urmapx_index_seqdata_size(const urmapx_index *);
uint32_t urmapx_index_seq_count(const urmapx_index *);
const char *urmapx_index_label(const urmapx_index *, uint32_t i);
uint32_t urmapx_index_seq_length(const urmapx_index *, uint32_t i);
uint32_t urmapx_index_seq_offset(const urmapx_index *, uint32_t i);

/* ---- mapping context: one per (index, device, host thread); replaces State1 + SetUFI ---- */
int urmapx_ctx_create(const urmapx_index *, int device, const urmapx_params *, urmapx_ctx **out);
void urmapx_ctx_destroy(urmapx_ctx *);

/* State1::Search over a batch of single-end reads held in HOST memory.
 * bases: concatenated ASCII reads (exactly as in the FASTQ); offs[n+1] byte offsets.
 * results[n] and path_ops[path_cap] are caller-owned host arrays; *path_used receives the
 * number of arena entries written.  Returns URMAPX_E_UNSUPPORTED (results still filled,
 * offending reads carry status bits) if any read fell outside the device path's domain. */
int urmapx_map_se(urmapx_ctx *, const uint8_t *bases, const uint64_t *offs, uint32_t n, urmapx_result *results,
                  urmapx_path_op *path_ops, size_t path_cap, size_t *path_used);

/* State2::Search (search2.cpp:59-73; -map2, method 4) over a batch of read PAIRS in host memory: reads 2i and 2i+1 of
 * (bases, offs) are the two mates of pair i (R1, R2).  results[2*npairs]: per mate the hit AdjustTopHitsAndMapqs
 * (search2.cpp:8-57) settled on, after SetMappedPos; `score` is that hit's score.  Flags, RNEXT/PNEXT and TLEN are
 * host-side text (urmapx_sam_pe).  Device-domain limits as urmapx_map_se, plus read length <= 279 (the reference
 * keeps pending seed positions in a byte, state1.h:86-87, and crashes on longer pairs). */
int urmapx_map_pe(urmapx_ctx *, const uint8_t *bases, const uint64_t *offs, uint32_t npairs, urmapx_result *results,
                  urmapx_path_op *path_ops, size_t path_cap, size_t *path_used);

/* Same with inputs and outputs already resident in HBM of the ctx's device (no PCIe in the call):
 * d_bases, d_offs (uint64[n+1]), d_results[n], d_path_ops[n*URMAPX_MAX_PATH_OPS], d_path_used (uint32).
 * Asynchronous on the ctx stream; urmapx_ctx_sync() waits. total_bases = offs[n]. */
int urmapx_map_se_device(urmapx_ctx *, const void *d_bases, const void *d_offs, uint32_t n, uint64_t total_bases,
                         uint32_t max_read_len, void *d_results, void *d_path_ops, void *d_path_used);
/* `urmap -map2 ... -veryfast`: State2 method 5 = Search5 (search2m5.cpp:9-156) with band radius 4 (map2.cpp:17-21).
 * The context's State1 parameters stay method 6, as in the reference (map2.cpp:15-16). */
int urmapx_ctx_set_pe_veryfast(urmapx_ctx *, int on);
/* Paired form of urmapx_map_se_device: 2*npairs reads resident in HBM, mates interleaved. */
int urmapx_map_pe_device(urmapx_ctx *, const void *d_bases, const void *d_offs, uint32_t npairs, uint64_t total_bases,
                         uint32_t max_read_len, void *d_results, void *d_path_ops, void *d_path_used);
int urmapx_ctx_sync(urmapx_ctx *);
/* Device time (ms, HIP events on the ctx stream) of the two kernels in the most recent *_device call that has
 * completed: [0] seed+probe, [1] search/extend. */
int urmapx_ctx_last_kernel_ms(urmapx_ctx *, float ms[2]);
/* A single-end call is: the search kernel (seed + probe + Search_Lo's phases 1-5), the flank-DP launches of phase 6, phase
 * 6's ordered part (finalize); the same three for the few reads whose hit / HSP lists outgrew the first pass's; the
 * general kernel over whatever both passes left flagged.  Device times in ms: [0] search, [1] its DP launches summed,
 * [2] its finalize launches summed, [3..5] the second pass likewise, [6] the general kernel. */
int urmapx_ctx_stage_ms(urmapx_ctx *, float ms[7]);
/* The same call's phase-6 launches one by one (first pass): ms[2*r] = the DP launch of round r, ms[2*r+1] = the finalize
 * launch behind it; *rounds = how many rounds the call had (3 or 4: urmapx_ctx_dp_rounds). */
int urmapx_ctx_round_ms(urmapx_ctx *, float ms[16], int *rounds);
/* The rounds of that call: round r = the HSPs lo[r] <= k < lo[r + 1] of a read (the last round is open ended: lo[rounds] = UINT32_MAX).
 * Reads of up to 192 bases: [0,2) [2,16) [16,..); longer reads: [0,2) [2,8) [8,32) [32,..) (round 5). */
int urmapx_ctx_dp_rounds(urmapx_ctx *, uint32_t lo[8], int *rounds);
/* Round 5: phase 3 of Search_Lo (AlignHSP when the best HSP of phases 1-2 is long, search1m6.cpp:162-171) is parked like phase 6:
 * the search stage ([0] above) is then three launches -- ms[0] the first search launch (seed + probe + phases 1-2 for every read,
 * phases 4-5 for the reads with nothing to align in phase 3), ms[1] phase 3's flank-DP launch, ms[2] the search launch over the reads
 * parked at phase 3 (replay of AlignHSP's bookkeeping, phases 4-5).  stats[0] = DpJobs made for phase 3, stats[1] = reads parked there.
 * All zero when phase 3 ran inside the search kernel (the context records which it was; round 6), which is the DEFAULT: measured at hg38 scale
 * the three launches take 6 % longer than the one (profiles/r5/README.md).  URMAPX_PARK_PHASE3=1 in the environment -- set BEFORE the index is
 * uploaded: the parked variant needs the row layout, which an upload without the knob drops once slot16 is built -- turns the parking on (reads
 * of up to 320 bases). */
int urmapx_ctx_phase3(urmapx_ctx *, float ms[3], uint32_t stats[2]);
/* Statistics of the same call, per pass (4 numbers each): HSPs handed to the DP launches, reads they belong to, how many
 * of those DPs the ordered replay of AlignHSP (alignhsp.cpp:60-172) looked at, and how many were dropped before their DP
 * because the penalty cap had fallen far enough by their round. */
int urmapx_ctx_dp_stats(urmapx_ctx *, uint32_t out[8]);

/* Diagnostic: shader cycles spent per phase by the last search kernel, summed over wavefronts:
 * [0] setup, [1] phases 1+2, [2] phase 3, [3] chain walks, [4] phase 4, [5] phase 5, [6] phase 6, [7] output;
 * inside the candidate batches of phases 1,2,4,5: [8] locate+fetch, [9] window compare, [10] x-drop walks, [11] ordered part.
 * Only collected when URMAPX_PHASE_STATS is set in the environment (otherwise all zero / E_ARG). */
int urmapx_ctx_phase_cycles(urmapx_ctx *, uint64_t out[12]);
/* Diagnostic, same switch: shader cycles / 16 spent on each of the first n reads of the last single-end call (the cost
 * of a read is heavy-tailed; this is how the tail is looked at). */
int urmapx_ctx_read_cycles(urmapx_ctx *, uint32_t *out, uint32_t n);

/* ---- stage-level entry points (same device code the batch call runs; used by parity tests and bench) ---- */
/* State1::SetSlotsVec (state1.cpp:396-438) + UFIndex::GetBlob (ufindex.h:184-187) for both strands of every read.
 * Host arrays; per read r, entries [2*offs[r], 2*offs[r]+L) are the plus strand by query position and
 * [2*offs[r]+L, 2*offs[r]+2L) the minus strand (positions > L-W unused).  slots: UINT64_MAX = no k-mer. */
int urmapx_seed_probe(urmapx_ctx *, const uint8_t *bases, const uint64_t *offs, uint32_t n, uint64_t *slots,
                      uint8_t *tallies, uint32_t *positions);
/* State1::Viterbi (viterbi.cpp:11-261) + TraceBackBitMem for a batch of (A,B) pairs.
 * a/b: concatenated sequences with offsets; flags bit0 = Left, bit1 = Right.  Outputs per problem: score,
 * status (URMAPX_ST_*), and the run-length path in ops[i*URMAPX_MAX_PATH_OPS ..] with nops[i] entries. */
int urmapx_viterbi_batch(urmapx_ctx *, const uint8_t *a, const uint32_t *a_offs, const uint8_t *b,
                         const uint32_t *b_offs, const uint8_t *flags, uint32_t n, float *scores, uint8_t *status,
                         urmapx_path_op *ops, uint16_t *nops);

/* The same stage over reads already resident in HBM of the ctx's device, nothing copied back (measurement: the probe launch alone,
 * *ms = its time on the ctx stream; inside urmapx_map_se* the probe is a stage of the search kernel).  Results stay in the context's
 * probe arrays. */
int urmapx_seed_probe_device(urmapx_ctx *, const void *d_bases, const void *d_offs, uint32_t n, uint64_t total_bases,
                             uint32_t max_read_len, float *ms);

/* Measurement aid (no reference counterpart): n_loads independent random 5-byte slot reads over the resident slot
 * table and nothing else -- the random-access ceiling of this table on this device, which bench.py reports next to
 * the probe kernel's rate (SURVEY.md section 8d asks for the denominator to be measured, not assumed). */
int urmapx_ctx_gather_microbench(urmapx_ctx *, uint64_t n_loads, double *loads_per_s);

/* ---- index construction (host side; the command line's -make_ufi) ---- */
/* cmd_make_ufi (ufindexio.cpp:117-179): FASTA -> .ufi, byte-identical to the reference's for the same slot count.
 * slots is mandatory here; the command line applies the reference's default, GetPrime(file_size / 0.6)
 * (prime.cpp:11-21), when -slots is absent. */
int urmapx_make_ufi(const char *fasta_path, const char *ufi_path, uint32_t word_length, uint32_t max_ix, uint64_t slots);
/* UFIndex::MakeIndex (ufindex.cpp:83-151) on an already concatenated upper-case sequence store; blob: 5*slots bytes. */
int urmapx_build_slots(const uint8_t *seqdata, uint32_t seqdata_size, uint32_t word_length, uint32_t max_ix,
                       uint64_t slots, uint8_t *blob, uint32_t *truncated_out);

/* The same two with the data-parallel passes on the GPU (both strands' per-slot counts, ufindex.cpp:338-408; the first
 * indexed position of every slot; the head slots; the remaining positions as a list in genome order) and only the
 * order-dependent inserts (UpdateSlot / FindFreeSlot, ufindex.cpp:194-322,987-1000) on the host.  Byte-identical output.
 * d_seqdata: the sequence store already resident on `device`, or NULL (then the host array seqdata is uploaded). */
int urmapx_make_ufi_gpu(int device, const char *fasta_path, const char *ufi_path, uint32_t word_length, uint32_t max_ix, uint64_t slots);
/* Either builder (device < 0: host) with cmd_make_ufi's label option: by default sequence labels are cut at the first
 * white space (ufindexio.cpp:123-128); URMAPX_UFI_KEEP_LABELS = the reference's -notrunclabels. */
#define URMAPX_UFI_KEEP_LABELS 1u
int urmapx_make_ufi_opts(int device, const char *fasta_path, const char *ufi_path, uint32_t word_length, uint32_t max_ix,
                         uint64_t slots, unsigned flags);
int urmapx_build_slots_gpu(int device, const uint8_t *seqdata, const void *d_seqdata, uint32_t seqdata_size, uint32_t word_length,
                           uint32_t max_ix, uint64_t slots, uint8_t *blob, uint32_t *truncated_out);

/* ---- k-mer bit-vector read filter: -make_bitvec, -search_bitvec, -search_bitvec2 (makebitvec.cpp, searchbitvec.cpp,
 * searchbitvec2.cpp, bitvec.{h,cpp}) ---- */
/* A table of 4^W bits, one per W-mer, resident in the HBM of one device.  A W-mer is W letters of g_CharToLetterNucleo (ACGTU and
 * acgtu -> 0..3, every other byte invalid), 2 bits each, the first letter most significant.  Strand 1 of a sequence is its reverse
 * complement by characters (g_CharToCompChar: 'U' -> 'A', 'u' -> '?', which is invalid).  As in the reference's loops
 * (makebitvec.cpp:29, searchbitvec.cpp:28), a sequence of length L contributes, on each strand, only the words that START at
 * 0 .. L-2W+1: a sequence shorter than 2W-1 has none.  Where the reference is undefined -- a sequence or read shorter than W-1, whose
 * unsigned loop bound wraps -- this build defines it: such a sequence contributes nothing and such a read is never found.
 * .bv file: uint32 magic URMAPX_BV_MAGIC ("01VB" as bytes), uint32 W, 4^W/8 bytes of bits; bit n = byte[n >> 3] & (1 << (n & 7)). */
typedef struct urmapx_bitvec urmapx_bitvec;
#define URMAPX_BV_MAGIC 0x42563130u
#define URMAPX_BV_MIN_W 2
#define URMAPX_BV_MAX_W 20 /* the table alone is 128 GiB here; W outside 2..20 is URMAPX_E_UNSUPPORTED */
/* Build on `device`: set the bit of every word of the sequences seqs[offs[i] .. offs[i+1]) (i < n), both strands; then clear that of
 * every word of excl[excl_offs[i] .. excl_offs[i+1]) (i < n_excl; excl may be NULL with n_excl = 0).  Host arrays.  counts (may be NULL):
 * [0] words included (the popcount after the first pass), [1] words excluded ([0] minus the popcount after the second). */
int urmapx_bitvec_build(int device, const uint8_t *seqs, const uint64_t *offs, uint32_t n, const uint8_t *excl, const uint64_t *excl_offs,
                        uint32_t n_excl, uint32_t word_length, urmapx_bitvec **out, uint64_t counts[2]);
/* A .bv file straight into the HBM of `device` (page-locked pieces, no host copy of the bits).  URMAPX_E_FORMAT: bad magic or a file
 * shorter than its header says; URMAPX_E_UNSUPPORTED: W outside 2..20. */
int urmapx_bitvec_open(const char *bv_path, int device, urmapx_bitvec **out);
/* Copy caller-owned host bits (4^W/8 bytes, the .bv layout) to `device`. */
int urmapx_bitvec_wrap_host(int device, uint32_t word_length, const uint8_t *bits, urmapx_bitvec **out);
int urmapx_bitvec_save(const urmapx_bitvec *, const char *bv_path);
/* the 4^W/8 bytes of bits to a host array of at least that many bytes */
int urmapx_bitvec_download(const urmapx_bitvec *, uint8_t *bits, uint64_t cap);
uint32_t urmapx_bitvec_word_length(const urmapx_bitvec *);
uint64_t urmapx_bitvec_bytes(const urmapx_bitvec *);
int urmapx_bitvec_popcount(const urmapx_bitvec *, uint64_t *out);
/* SearchBitVec1 (searchbitvec.cpp:17-55) per read: verdicts[i] = 1 if a strand-0 word of read i is set, else 2 if a strand-1 word
 * is, else 0.  Reads of any length (concatenated bases, offs[n+1]); host arrays, synchronous. */
int urmapx_bitvec_search(urmapx_bitvec *, const uint8_t *bases, const uint64_t *offs, uint32_t n, uint8_t *verdicts);
/* The same over reads resident in HBM of the bit vector's device (the d_bases / d_offs convention of urmapx_map_se_device,
 * d_offs[0] = 0), verdicts to d_verdicts[n]; asynchronous on the bit vector's stream, urmapx_bitvec_sync waits. */
int urmapx_bitvec_search_device(urmapx_bitvec *, const void *d_bases, const void *d_offs, uint32_t n, void *d_verdicts);
int urmapx_bitvec_sync(urmapx_bitvec *);
/* device time (ms, HIP events) of the last build's include and exclude launches [0], [1] and of the last completed search launch [2] */
int urmapx_bitvec_last_ms(urmapx_bitvec *, float ms[3]);
void urmapx_bitvec_close(urmapx_bitvec *);
/* cmd_make_bitvec (makebitvec.cpp:72-106): both FASTA files read as SeqDB::FromFasta does (case kept), the table built on `device`
 * and written to bv_path.  excl_fa is required, as in the reference ("Missing input file name"). */
int urmapx_make_bitvec(int device, const char *ref_fa, const char *excl_fa, uint32_t word_length, const char *bv_path, uint64_t counts[2]);
/* cmd_search_bitvec / cmd_search_bitvec2: FASTQ (plain or .gz, the urmapx_fastq_* rules) -> the records that were found, in input
 * order, each as FASTQSeqSource left it (a read found on strand 1 reverse-complemented with its quality string reversed).  fq2 NULL:
 * single-end into out1.  Else pairs: a pair is written (mate 1 to out1, mate 2 to out2) when either mate is found; a mate that was not
 * found has been through both scans, so it is written reverse-complemented.  Labels whole unless URMAPX_BV_TRUNC_LABELS (cut at the
 * first white space).  counts (may be NULL): [0] reads (pairs) found, [1] reads (pairs) read.  URMAPX_E_FORMAT with a message in err
 * for malformed FASTQ or mate files of unequal record counts. */
#define URMAPX_BV_TRUNC_LABELS 1u
int urmapx_search_bitvec_files(urmapx_bitvec *, const char *fq1, const char *fq2, const char *out1, const char *out2, unsigned flags,
                               uint64_t counts[2], char *err, size_t errcap);

/* ---- host-side text (no device involved) ---- */
/* One SAM record of a single-end read: State1::SetSAM / SetSAM_Unmapped (setsam.cpp:12-207) with Flags = 0 as
 * State1::Output1 passes (output1.cpp:13), CIGAR per state1.cpp:707-734 + cigar.cpp.  path_ops = the batch arena.
 * Writes at most cap bytes (no NUL); returns the record length, or 0 if cap is too small. */
size_t urmapx_sam_se(const urmapx_index *, const urmapx_result *r, const urmapx_path_op *path_ops, const char *label,
                     const uint8_t *seq, const uint8_t *qual, uint32_t read_len, char *buf, size_t cap);
/* The two SAM records of a read pair: State2::SetSAM2 / GetPairedFlags (output2.cpp:18-128) + SetSAM. */
size_t urmapx_sam_pe(const urmapx_index *, const urmapx_result *r1, const urmapx_result *r2, const urmapx_path_op *path_ops,
                     const char *label1, const uint8_t *seq1, const uint8_t *qual1, uint32_t len1, const char *label2,
                     const uint8_t *seq2, const uint8_t *qual2, uint32_t len2, char *buf, size_t cap);
/* @SQ lines of State1::WriteSAMHeader (state1.cpp:736-748); same return convention. */
size_t urmapx_sam_header_sq(const urmapx_index *, char *buf, size_t cap);

/* ---- paired-end summary (-tabbedout) ---- */
/* What State2::OutputTab2 (outputtab2.cpp:85-120) reads beyond the two mates' results: each mate's m_TopHit as the
 * pair stage left it (BEFORE SetMappedPos, which SetSAM2 applies only when SAM output is on) and m_SecondHit, which
 * AdjustTopHitsAndMapqs sets from the second-best pair (search2.cpp:49-56).  UINT32_MAX = no such hit. */
typedef struct urmapx_pair_info {
	uint32_t top_db[2], second_db[2];
	int16_t top_score[2], second_score[2];
	uint8_t top_plus[2], second_plus[2];
} urmapx_pair_info;
/* on != 0: urmapx_map_pe / urmapx_map_pe_device also record one urmapx_pair_info per pair (device side) */
int urmapx_ctx_set_pair_info(urmapx_ctx *, int on);
/* copies the records of the last paired-end call (npairs of them) to the host */
int urmapx_ctx_get_pair_info(urmapx_ctx *, urmapx_pair_info *out, uint32_t npairs);
/* One line of the reference's -tabbedout file: pair label, top pair position(s), the two MAPQs, second pair or '*',
 * and "TL=..;Score=..;" when all four hits exist.  sam_on: the reference's line differs when -samout is also given
 * (a top hit overhanging its sequence has been cleared by then).  Returns the length written, 0 if cap is too small. */
size_t urmapx_tab_pe(const urmapx_index *, const urmapx_result *r1, const urmapx_result *r2, const urmapx_pair_info *info,
                     const char *label1, uint32_t len1, uint32_t len2, int sam_on, char *buf, size_t cap);

/* ---- file to file: cmd_map / cmd_map2 (map.cpp:27-67, map2.cpp:39-90) as a library call ---- */
typedef struct urmapx_map_options {
	int first_gpu;      /* -gpu D */
	int gpus;           /* -gpus N: devices D..D+N-1, one replica of the index on each; 0 = 1 */
	int streams;        /* -streams K: mapping contexts per device (copies of one overlap kernels of another); 0 = 2 */
	int host_threads;   /* -threads: FASTQ parsing and SAM formatting; 0 = min(16, hardware threads) */
	uint32_t batch;     /* reads per batch; 0 = the library chooses: 262 144, up to 524 288 for files large enough to give every lane four chunks */
	int veryfast;       /* -veryfast: State1 method 7 for -map, State2 method 5 for -map2 */
	unsigned minq;      /* -minq (only -map2 reads it, map2.cpp:76) */
	const char *cmdline; /* text after CL: in the @PG line (NULL: empty) */
	/* round 4 (0 = the reference's behaviour: one SAM file) */
	int sam_shards;     /* -samshards N: the SAM text goes to N files samout.0 .. samout.N-1, shard s = the records of the s-th
	                     * N-th of the input (cut at a record), written by its own pipeline (reader, lanes, writer) on its own
	                     * share of the devices; the header is in shard 0, so `cat samout.0 .. samout.N-1` is byte for byte what one
	                     * file would hold.  Plain (seekable, not .gz) input only: other input is mapped by ONE
	                     * pipeline over all the devices into shard 0, the other shards stay empty.  -tabbedout is split the same way
	                     * (tabout.0 ..).  Needs samout (URMAPX_E_ARG without); N in 1..64 must divide gpus or be a multiple of it.  A failed
	                     * run removes the shard files it wrote */
	int discard_sam;    /* measurement: the SAM text is made and copied to the host, then dropped instead of written (report.medium
	                     * "discarded"): what the device lanes sustain when the output medium is not in the way */
	int bgzf;           /* -bgzf: samout is a BGZF file (see "BGZF output" below): the header and every chunk's text as gzip members of their
	                     * own, deflated on the device for the chunks the device formats and by urmapx_bgzf_compress_host for the others, the
	                     * end-of-file member last.  With sam_shards every shard is such a file.  0: plain text, whatever samout is called.
	                     * Text from the device is cut every 65 280 bytes within a chunk.  Text the host formats (-host, chunks handed back)
	                     * is compressed per host thread, each thread's share of a batch as members of its own: valid BGZF that inflates to
	                     * the same text, but there the members' cuts, the file's bytes and its size depend on host_threads */
	int bam;            /* -bamout: samout is a BAM file (see "BAM output" below): the header block and every chunk's alignment records inside
	                     * BGZF members framed as under bgzf (which is implied; setting both is URMAPX_E_ARG), the records encoded on the
	                     * device for the chunks the device formats and by urmapx_bam_se / _pe for the others.  With sam_shards every shard is
	                     * a complete BAM file with the header.  A QNAME over 254 bytes does not fit a BAM record: URMAPX_E_FORMAT, the read
	                     * named in err.  0: SAM */
	int bam_sort;       /* -sort (with bam): the records of samout in coordinate order (see "Sorted BAM output" below) and their index in
	                     * samout + ".bai".  The header text begins with "@HD\tVN:1.6\tSO:coordinate".  The lanes hand over raw records,
	                     * which are kept in host memory in input order; behind the last one they go to first_gpu once (urmapx_bam_sort; when
	                     * no chunk took the device road, urmapx_bam_sort_host) and the file and its index are written: header block in a
	                     * member of its own, the sorted stream cut every 65 280 bytes, the end-of-file member.  The inflated bytes do not
	                     * depend on gpus, streams, batch or host_threads.  If the device has no room (urmapx_bam_sort_device_bytes) the kept
	                     * lanes are let go first; then the records are streamed through the device with the memory that is free
	                     * (urmapx_bam_sort_external), and only where the per-record arrays and one slice do not fit either the run ends
	                     * with URMAPX_E_NOMEM, the least bytes needed and the bytes free in err.  URMAPX_E_ARG without bam, with
	                     * sam_shards > 1 or with discard_sam; samout must be a regular file.  A failed run removes both files */
	unsigned tags;      /* -tags: URMAPX_TAG_NM | _MD | _AS, the optional fields of every mapped record (see "Optional fields" below); 0: none */
	const char *read_group; /* -rg: a complete @RG header line, tabs real, with an ID: field (urmapx_read_group_id); it goes into the header in
	                     * front of the @PG line and every record gets RG:Z:<ID>.  NULL: neither.  URMAPX_E_ARG with the reason in err for a
	                     * line urmapx_read_group_id refuses and for tag bits outside URMAPX_TAG_ALL */
	int markdup;        /* -markdup (with bam_sort): flag 0x400 of every record says whether it is a duplicate (see "Duplicate marking" below),
	                     * decided on first_gpu while the kept records lie there for the sort (urmapx_bam_sort_markdup; on the host road
	                     * urmapx_bam_sort_markdup_host).  Only the flag half-words differ from the run without it: the order, the cuts and
	                     * the index stay.  The counters go to the report.  URMAPX_E_ARG with the reason in err without bam_sort */
	uint64_t sort_mem;  /* -sortmem (with bam_sort): the device memory the sort may take, in bytes.  The sort is planned from it directly
	                     * (urmapx_bam_sort_plan_for): in core where that fits, else streamed through the device in as few partitions as
	                     * fit (urmapx_bam_sort_external); URMAPX_E_NOMEM naming the least it takes where even one slice does not.  0: in
	                     * core when the device has room, else streamed with what is free.  No effect on the host road.  URMAPX_E_ARG
	                     * without bam_sort */
	const char *depth_out; /* -depth (with bam_sort): a bedGraph file of the per-base depth of the records as the BAM file holds them --
	                     * under markdup without the duplicates --, taken on first_gpu while the records lie there for the sort (see "Depth"
	                     * below; urmapx_bam_sort_with, on the host road urmapx_bam_sort_with_host).  The BAM file and its index are those
	                     * of the run without it but for the @PG line.  The depth arrays come off sort_mem (or off what is free) before the
	                     * sort is planned; URMAPX_E_NOMEM naming the least budget where they do not fit.  The totals go to the report, the
	                     * table per reference to urmapx_map_depth_summary.  NULL: none.  URMAPX_E_ARG without bam_sort, and for a name
	                     * that is samout's or its index's.  A failed run removes the file with the other two */
	uint32_t depth_mapq; /* -depth_mapq (with depth_out): records with a MAPQ below it do not count; 0 .. 255 */
	const char *stats_out; /* -stats (with bam_sort): a text file of the alignment statistics of the records as the BAM file holds them -- under
	                     * markdup with the marking's bit 0x400 --, counted on first_gpu where the depth is taken (see "Stats" below;
	                     * urmapx_bam_sort_with, on the host road urmapx_bam_sort_with_host); its second line carries cmdline.  The BAM file
	                     * and its index are those of the run without it but for the @PG line.  The tables come off sort_mem (or off
	                     * what is free) with the depth's arrays before the sort is planned.  A few totals go to the report.  NULL: none.
	                     * URMAPX_E_ARG without bam_sort, for an empty name and for a name that is samout's, its index's or depth_out's.
	                     * A failed run removes the file with the others */
	const char *vcf_out;   /* -vcfout (with bam_sort): a sites-only VCF 4.2 file of the columns where the records as the BAM file holds them --
	                     * under markdup without the marked duplicates -- show a base other than the reference's (see "Pileup" below),
	                     * counted on first_gpu where the depth is taken (urmapx_bam_sort_with, on the host road urmapx_bam_sort_with_host).
	                     * The reference bases are the index's sequence store, read in place where it is resident on first_gpu and fetched
	                     * once (urmapx_index_fetch_spans) where it is not.  Its ##urmapCommand line carries cmdline.  The BAM file and its
	                     * index are those of the run without it but for the @PG line.  The counters (16 bytes a reference base) come off
	                     * sort_mem (or off what is free) with the depth's and the statistics' arrays before the sort is planned.  NULL: none.
	                     * URMAPX_E_ARG without bam_sort, for an empty name and for a name that is samout's, its index's, depth_out's or
	                     * stats_out's.  A failed run removes the file with the others */
	uint32_t vcf_mapq;     /* -vcf_mapq (with vcf_out): records with a MAPQ below it do not count; 0 .. 255 */
	uint32_t vcf_baseq;    /* -vcf_baseq: bases with a quality below it do not count; 0 .. 255 */
	uint32_t vcf_min_alt;  /* -vcf_min_alt: the least count of an alternative allele; 1 or more (URMAPX_E_ARG for 0 with vcf_out) */
	uint32_t vcf_min_pct;  /* -vcf_min_pct: its least share of DP in per cent; 0 .. 100.  All four are taken as they stand: the defaults
	                     * (0, 13, 3, 10) are the command line's and api.py's */
} urmapx_map_options;
typedef struct urmapx_map_report {  /* State1::HitStats' counters (state1.cpp:593-632) and where the time went */
	uint64_t reads, mapped_q, mapped_lowq, unmapped, unsupported;
	double seconds;                                  /* first read parsed .. last SAM byte written (index load excluded) */
	double parse_s, gpu_s, format_s, write_s;        /* busy seconds per stage (gpu: summed over the lanes) */
	int host_threads, lanes;
	int write_threads;                               /* threads sharing one piece's pwrite (1 on tmpfs, up to 4 on a disk file system) */
	int text_on_device;                              /* 1: FASTQ bytes went to the device and SAM bytes came back (plain or .gz files) */
	uint64_t input_bytes;                            /* uncompressed FASTQ bytes that took that road (for .gz: parse_s is the inflater's busy time) */
	char medium[24];                                 /* what the SAM file lives on: "tmpfs", "disk file system", "pipe", "none", "discarded" */
	/* round 4: where a device lane's time goes (seconds summed over the chunks of all lanes, from events on the lanes' streams;
	 * text phase only): FASTQ bytes to the device, line ends / record checks / base copy, the mapping kernels, SAM lengths + text,
	 * SAM bytes back */
	double dev_h2d_s, dev_parse_s, dev_map_s, dev_format_s, dev_d2h_s;
	int shards;                                      /* SAM files written (1 unless sam_shards) */
	char placement[256];                             /* where the run's threads were put: "gpu0@node1 gpu1@node1; reader+writer@node1" per pipeline
	                                                  * (shards separated by " | "); @any = not pinned (no NUMA node known for the device).  A lane's
	                                                  * host thread runs on the CPUs of its device's NUMA node; reader and writer too when all devices
	                                                  * of the pipeline share one node */
	double shard_scan_s;                             /* sam_shards: seconds spent cutting the input at record starts (pairs: counting the lines that
	                                                  * place the cuts of the mates' file); inside `seconds` */
	double dev_map_search_s, dev_map_dp_s;           /* of dev_map_s (single-end): the search launches; phase 6's dp + finalize launches */
	double map_enqueue_s;                            /* host seconds the lanes spent enqueueing mapping launches (a lane thread that is not scheduled shows here) */
	double alloc_dev_s, alloc_pinned_s;              /* seconds all threads of the call spent in hipMalloc / hipFree of the lanes' device arrays, and in
	                                                  * hipHostMalloc / hipHostFree of page-locked chunk buffers (kept for the next call: 0 calls when warm) */
	uint32_t alloc_dev_calls, alloc_pinned_calls;
	uint64_t sam_text_bytes, sam_file_bytes;         /* SAM text (bam: header block and records) made, bytes written to samout: equal unless bgzf / bam */
	double sort_s;                                   /* bam_sort: last record mapped .. last byte of samout and samout.bai written; inside `seconds` */
	uint64_t pairs_examined, pairs_duplicate, fragments_examined, fragments_duplicate;  /* markdup: urmapx_markdup_stats of the run's records */
	double markdup_s;                                /* markdup: the marking's share of sort_s */
	uint32_t sort_partitions;                        /* bam_sort: partitions the sorted stream was made in on the external road; 0: in core (or the host) */
	double depth_s;                                  /* depth_out: the depth's share of sort_s (its arrays, the counting, scan, runs, text and the file) */
	uint64_t depth_runs, depth_covered, depth_bases; /* depth_out: lines of the file; columns with depth >= 1 and the sum of all depths, over all references */
	double stats_s;                                  /* stats_out: the statistics' share of sort_s (their tables, the counting, the text and the file) */
	uint64_t stats_reads, stats_mapped, stats_properly_paired, stats_duplicated, stats_insert_median;  /* stats_out: the SN lines of those names */
	double pileup_s;                                 /* vcf_out: the pileup's share of sort_s (its counters, the counting, the sites, the text and the file) */
	uint64_t pileup_sites;                           /* vcf_out: lines of the file behind its header */
	uint64_t pileup_records, pileup_alt_alleles;     /* vcf_out: records that counted (rule 1); ALT entries over all lines (the log line's numbers) */
} urmapx_map_report;
/* fastq2 NULL: single-end (-map); else the mates' file (-map2 ... -reverse).  samout / tabout may be NULL.  The index
 * needs its host arrays, or to be resident on first_gpu already (the other devices' replicas are then copied from there).  Batch b is mapped on device
 * b mod gpus; records are written in input order.  Returns URMAPX_E_UNSUPPORTED if reads fell outside the device
 * domain (report->unsupported of them), URMAPX_E_FORMAT with the reference's message in err for malformed FASTQ. */
int urmapx_map_files(urmapx_index *, const urmapx_map_options *, const char *fastq1, const char *fastq2, const char *samout,
                     const char *tabout, urmapx_map_report *report, char *err, size_t errcap);

/* What urmapx_map_files keeps for the next call of this process, and what lets go of it:
 *   - page-locked chunk buffers, up to 16 GiB of host memory (pinning a few hundred MB costs as much as mapping the chunk in it);
 *   - its lanes: up to 8 mapping contexts with their text stages, 2.5-3 GB of DEVICE memory each (DpJobs, parked states, path arena,
 *     the chunk's text both ways), keyed on index, device, parameters and the URMAPX_* environment -- a lane is kept only while an
 *     eighth of the device's memory is still free with it there, so a process that shares the device with another allocator (torch)
 *     sees at most that much held back.
 * urmapx_host_pool_trim() frees both; urmapx_index_close() destroys the lanes of its index; URMAPX_NO_LANE_POOL=1 keeps no lanes. */
void urmapx_host_pool_trim(void);
/* The table of the calling thread's last urmapx_map_files run with depth_out: one line per reference --
 * "name\tlength\treads\tcovered\tpercent covered\tmean depth\tmean MAPQ\n", the percentage and the means with two decimals (0.00 for a
 * reference without columns or reads) -- under a header line that names the columns.  "" after a run without depth_out.  The text
 * is the library's until the thread's next run. */
const char *urmapx_map_depth_summary(void);

/* ---- FASTQ bytes in, SAM bytes out (both text stages of -map on the device) ---- */
/* One chunk of a FASTQ file, cut after a record's last '\n', goes to the device as it lies in the file; line ends,
 * record checks (FASTQSeqSource::GetNextLo, fastqseqsource.cpp:9-116), State1::Search and the SAM records
 * (State1::SetSAM / SetSAM_Unmapped with output1.cpp:13's arguments, setsam.cpp:12-207) run there and the records' text
 * comes back in input order.  A chunk the device parser does not take as it is ('\r', blank or missing lines, a
 * malformed record, a target label over 160 bytes) is handed back untouched with report.reason set: the caller runs it
 * through urmapx_fastq_* / urmapx_sam_se, which reproduce the reference's handling and messages. */
typedef struct urmapx_text urmapx_text;
#define URMAPX_TEXT_OK 0
#define URMAPX_TEXT_CR 1          /* a '\r' in the chunk */
#define URMAPX_TEXT_RAGGED 2      /* line count not a multiple of four, or no '\n' at the end of the chunk */
#define URMAPX_TEXT_BAD_RECORD 3  /* '@' missing, a byte that is not a letter, #bases != #quals, blank line */
#define URMAPX_TEXT_LONG_NAME 4   /* target label longer than the device formatter takes */
#define URMAPX_TEXT_SAM_CAP 5     /* sam_cap < report.sam_bytes: the chunk is mapped, its text waits for urmapx_text_fetch_sam */
#define URMAPX_TEXT_TOO_LARGE 6   /* chunk over 1 GiB, or its SAM text over 4 GiB */
#define URMAPX_TEXT_UNEQUAL 7     /* pairs: the two chunks do not hold the same number of records */
#define URMAPX_TEXT_INTERNAL 8    /* the device formatter's two passes disagreed on a record length (never expected): text not used */
#define URMAPX_TEXT_DEFERRED 9    /* urmapx_text_set_deferred: the chunk is mapped and counted, its text is on its way (urmapx_text_wait) */
typedef struct urmapx_text_report {
	uint32_t records;   /* reads of the chunk */
	uint32_t reason;    /* URMAPX_TEXT_*; non-zero: nothing was written */
	uint64_t sam_bytes; /* bytes of SAM text (written, or needed when reason is URMAPX_TEXT_SAM_CAP) */
	uint64_t mapped_q, mapped_lowq, unmapped, unsupported; /* State1::HitStats' counters (output1.cpp:20-30) against minq */
	float ms_h2d, ms_parse, ms_map, ms_format, ms_d2h;     /* the chunk on its stream, by events: copy in, parse, map, SAM text, copy out */
	float ms_map_search, ms_map_dp;                        /* of ms_map (single-end): the search launch; phase 6's dp + finalize launches */
	float ms_map_enqueue;                                  /* host time spent enqueueing the mapping launches (no wait inside: all of it is the calling thread) */
	uint64_t sam_text_bytes;                               /* bytes of SAM text (urmapx_text_set_bam: of BAM records) made; differs from sam_bytes only
	                                                        * under urmapx_text_set_bgzf */
} urmapx_text_report;
/* One per mapping context; calls on it run on the context's stream (one thread at a time per context). */
int urmapx_text_create(urmapx_ctx *, urmapx_text **out);
void urmapx_text_destroy(urmapx_text *);
/* fastq[fastq_bytes] and sam[sam_cap] are host arrays (page-locked ones cross PCIe without a staging copy). */
int urmapx_text_map_se(urmapx_text *, const char *fastq, size_t fastq_bytes, unsigned minq, char *sam, size_t sam_cap,
                       urmapx_text_report *report);
/* Pairs (-map2): a chunk of each mate file holding the same number of records; record 2i and 2i+1 of the text are the
 * mates of pair i with SetSAM2's flags, RNEXT, PNEXT and TLEN (output2.cpp:18-128); report.records counts reads (2 per
 * pair).  -tabbedout lines: urmapx_text_fetch_pairs + urmapx_tab_pe. */
int urmapx_text_map_pe(urmapx_text *, const char *fastq1, size_t fastq1_bytes, const char *fastq2, size_t fastq2_bytes,
                       unsigned minq, char *sam, size_t sam_cap, urmapx_text_report *report);
/* The copy back as a stage of its own.  With deferred on, urmapx_text_map_se / _pe / _fetch_sam return once the chunk's SAM text
 * has been made on the device and its copy to `sam` has been ENQUEUED on a second stream (report.reason URMAPX_TEXT_DEFERRED;
 * records, sam_bytes, the counters and ms_h2d / ms_parse / ms_map* are final), so that the caller can hand the context its next
 * chunk while the text crosses PCIe; urmapx_text_wait then waits for the OLDEST such copy and returns that chunk's final report
 * (reason 0 or URMAPX_TEXT_INTERNAL, ms_format, ms_d2h) -- only then may `sam` be read.  At most two chunks are in flight per
 * context: map(i), map(i+1), wait(i), map(i+2), wait(i+1) ...; a third map call before a wait returns URMAPX_E_ARG.
 * Round 5: a lane of urmapx_map_files runs this way (the reference has no counterpart: its threads write records as they finish). */
int urmapx_text_set_deferred(urmapx_text *, int on);
int urmapx_text_wait(urmapx_text *, urmapx_text_report *report);
/* on != 0: the chunk's text is deflated on the device (urmapx_bgzf_compress_device on the context's stream, behind the kernel that
 * writes the text) and `sam` receives whole BGZF members, no end-of-file member: a chunk is not the end of a file.  report.sam_bytes
 * is then the compressed size, report.sam_text_bytes the text's, ms_format includes the compressor.  `sam` must hold
 * urmapx_bgzf_bound(text bytes) - 28: a smaller one gives URMAPX_TEXT_SAM_CAP with that number in sam_bytes, as for plain text.
 * Where the wait sits: the compressed size exists only once the compressor has run, so urmapx_text_map_se / _pe / _fetch_sam wait on the
 * context's stream for it (one 8-byte copy behind the compress launch) and only then enqueue the copy of exactly that many bytes -- on
 * the second stream when deferred, so the PCIe transfer still overlaps the next chunk; what no longer overlaps it is the text kernel and
 * the compressor of this chunk.  URMAPX_E_ARG while a chunk is in flight or waiting to be fetched. */
int urmapx_text_set_bgzf(urmapx_text *, int on);
/* on != 0: the chunk's output is its BAM alignment records (bam_kernel in text_gpu.hip; the layout under "BAM output" below) instead
 * of SAM text: no header block, records in input order, back to back.  With urmapx_text_set_bgzf off `sam` receives the raw records,
 * with it on BGZF members of them (a record may span members); report.sam_text_bytes is the uncompressed record bytes either way.
 * Deferred mode, URMAPX_TEXT_SAM_CAP and urmapx_text_fetch_sam as for text.  A chunk with a QNAME over 254 bytes is handed back
 * (URMAPX_TEXT_LONG_NAME).  URMAPX_E_ARG while a chunk is in flight or waiting to be fetched. */
int urmapx_text_set_bam(urmapx_text *, int on);
/* After URMAPX_TEXT_SAM_CAP: the text of the chunk just mapped into a buffer of at least report.sam_bytes (the search is
 * not run again).  URMAPX_E_ARG if no such chunk is waiting. */
int urmapx_text_fetch_sam(urmapx_text *, char *sam, size_t sam_cap, urmapx_text_report *report);
/* After urmapx_text_map_pe mapped a chunk (reason 0 or URMAPX_TEXT_SAM_CAP) on a context with urmapx_ctx_set_pair_info
 * on: what State2::OutputTab2 (outputtab2.cpp:85-120) needs for the chunk's -tabbedout lines, which the host formats with
 * urmapx_tab_pe -- the 2 * npairs results, the npairs pair records, the offset of the '\n' of every line of the FIRST
 * file's chunk (4 * npairs: pair i's label is the text between the '@' that starts line 4i and line_ends1[4i], its first
 * mate's length line_ends1[4i+1] - line_ends1[4i] - 1) and the second mates' lengths.  npairs must be report.records / 2. */
int urmapx_text_fetch_pairs(urmapx_text *, uint32_t npairs, urmapx_result *results, urmapx_pair_info *info, uint32_t *line_ends1,
                            uint32_t *lens2);

/* ---- FASTQ input (host) ---- */
/* Batch form of FASTQSeqSource::GetNextLo (fastqseqsource.cpp:9-116) over LineReader (linereader.cpp:14-113):
 * plain or .gz by suffix; '\r' dropped; a final unterminated line counts; blank lines only at end of file; the same
 * accept/reject rules and messages ('@' expected, letters only, #bases == #quals).  One reader per file. */
typedef struct urmapx_fastq urmapx_fastq;
int urmapx_fastq_open(const char *path, urmapx_fastq **out);
/* Reads up to max_reads records.  Returns the number read (0 at end of file) or URMAPX_E_FORMAT with the reference's
 * message in urmapx_fastq_error().  The arrays belong to the reader and stay valid until its next call:
 * bases/quals concatenated, offs[n+1]; labels (text after '@', NUL terminated) at label_data + label_offs[i]. */
int64_t urmapx_fastq_next(urmapx_fastq *, uint32_t max_reads, const uint8_t **bases, const uint8_t **quals,
                          const uint64_t **offs, const char **label_data, const uint64_t **label_offs);
const char *urmapx_fastq_error(const urmapx_fastq *);
void urmapx_fastq_close(urmapx_fastq *);

/* ---- .gz input (host) ---- */
/* The reference reads .gz files through zlib, one stream on one thread (linereader.cpp:54-113, gzipfileio.cpp).  urmapx_map_files
 * cuts a gzip stream into segments that several threads inflate side by side (urmap_amd/csrc/pgzip.h: each finds a deflate block
 * start behind its cut, decodes with the 32 KB in front of it unknown, the references into that window are filled in once the
 * segment in front is done; every member's CRC-32 and length are checked as zlib does).  This entry point runs that reader alone:
 * gz_path inflated to out_path, the bytes `gzip -dc` writes.  threads <= 0: all.  stats (optional): bytes written, bytes that
 * came by the parallel road, bytes that came through zlib (small files, one thread, input the parallel decoder hands over).
 * URMAPX_E_FORMAT: not gzip, truncated, or corrupt (what was decoded before the damage is in out_path, as with zlib). */
int urmapx_gunzip_file(const char *gz_path, const char *out_path, int threads, uint64_t stats[3]);
/* Which of the reader's vector paths this host runs: bit 0 = symbols to bytes 32 at a time (AVX2), bit 1 = CRC-32 by carry-less
 * multiplication (PCLMULQDQ; set only after the routine has reproduced zlib's crc32 on its self-test).  URMAPX_PGZIP_NO_SIMD=1: neither. */
int urmapx_pgzip_simd(void);

/* ---- BGZF output (-bgzf): gzip members of at most 65 280 bytes of text, each with the 'BC' extra field that holds its size ----
 * What bgzip / htslib write and `gzip -dc`, Python's gzip, samtools and bgzip -d read.  The input is cut every 65 280 bytes wherever
 * that falls; every piece becomes one member (18 bytes of header, one deflate block, CRC-32, ISIZE); with_eof appends htslib's 28-byte
 * empty member.  A piece that would not shrink is a stored block, so a member is at most its text + 31 bytes.
 * urmapx_bgzf_bound(n): the most n bytes can become, end-of-file member included. */
size_t urmapx_bgzf_bound(size_t n);
/* zlib's deflate (level 1) inside that framing, on the calling thread, no device.  URMAPX_E_ARG: cap < urmapx_bgzf_bound(n). */
int urmapx_bgzf_compress_host(const void *in, size_t n, void *out, size_t cap, size_t *used, int with_eof);
/* The device compressor (bgzf_gpu.hip): LZ77 matches within the piece (hash of 4 bytes, greedy), per-piece dynamic Huffman codes,
 * CRC-32 on the device; one workgroup per piece.  The same input gives the same bytes on every run.  Host arrays, synchronous.
 * URMAPX_E_NODEVICE without a usable device.  _timed: *ms = the compress launches alone, by events. */
int urmapx_bgzf_compress(int device, const void *in, size_t n, void *out, size_t cap, size_t *used, int with_eof);
int urmapx_bgzf_compress_timed(int device, const void *in, size_t n, void *out, size_t cap, size_t *used, int with_eof, float *ms);
/* Diagnostic: the compressor's code-length stage alone, on the device, by the function the piece kernel calls.  counts[n] of an alphabet
 * of n <= 286 symbols -> lengths[n] of a complete prefix code of at most maxbits (1..15) bits, 0 for a count of 0.  force2 != 0: with
 * fewer than two symbols in use the lowest unused ones count once (the distance and the code-length alphabet).  URMAPX_E_ARG: n < 2 or
 * > 286, maxbits outside 1..15, fewer than two symbols in use (after force2) or more than 2^maxbits, counts that sum past 2^32 - 1. */
int urmapx_bgzf_code_lengths(int device, const uint32_t *counts, uint32_t n, uint32_t maxbits, int force2, uint8_t *lengths);
/* The same with everything resident in the HBM of `device`, asynchronous on the stream the compressor was created with (a hipStream_t;
 * NULL: the default stream): d_in[n] -> d_out[out_cap >= urmapx_bgzf_bound(n)], the size to *d_used (device memory).  The compressor
 * object owns the launch's scratch (a staging slot per piece, 1024 token arenas of 255 KiB): one per stream, one call at a time. */
typedef struct urmapx_bgzf urmapx_bgzf;
int urmapx_bgzf_create(int device, void *stream, urmapx_bgzf **out);
void urmapx_bgzf_destroy(urmapx_bgzf *);
int urmapx_bgzf_compress_device(int device, const void *d_in, size_t n, void *d_out, size_t out_cap, uint64_t *d_used, int with_eof,
                                urmapx_bgzf *);

/* ---- BAM output (-bamout): SAM/BAM specification v1, section 4 ----
 * The file is BGZF (above); inside it the header block -- magic "BAM\1", l_text, the header text append_sam_header writes (@SQ lines,
 * the @PG line), n_ref, (l_name, name\0, l_ref) per sequence of the index in index order -- then one record per read, in input order.
 * A record carries exactly what the SAM record of the same read carries, field for field: refID / pos (-1 / -1 where the text has
 * '*' / 0), l_read_name = QNAME + NUL, mapq, bin = reg2bin(pos, pos + the reference bases the CIGAR spans, or pos + 1), the CIGAR runs
 * after the dangling-M polish as len << 4 | op, flag, l_seq, next_refID / next_pos from RNEXT ('=' is refID) / PNEXT, tlen, SEQ as
 * printed (reverse-complemented for a minus-strand hit) 4 bits a base through "=ACMGRSVTWYHKDBN" (either case; any other letter 15),
 * QUAL - 33 (0xFF throughout where the text has '*').  Optional fields only where asked for: NM, MD, AS and RG behind QUAL as aux fields
 * ("Optional fields" below), in the SAM text and here alike; without -tags / -rg a record ends at QUAL.
 * urmapx_bam_header: the uncompressed header block; returns its size and writes it if it fits cap (buf may be NULL to ask). */
size_t urmapx_bam_header(const urmapx_index *, const char *cmdline, void *buf, size_t cap);
/* The host encoders, arguments as urmapx_sam_se / _pe: one record, the two records of a pair.  Return the bytes written, 0 if they do
 * not fit cap, URMAPX_BAM_LONG_NAME if a QNAME is over 254 bytes (l_read_name is one byte; nothing is truncated).  The device encoder
 * (urmapx_text_set_bam) writes the same bytes for the same read. */
#define URMAPX_BAM_LONG_NAME ((size_t)-1)
size_t urmapx_bam_se(const urmapx_index *, const urmapx_result *r, const urmapx_path_op *path_ops, const char *label,
                     const uint8_t *seq, const uint8_t *qual, uint32_t read_len, char *buf, size_t cap);
size_t urmapx_bam_pe(const urmapx_index *, const urmapx_result *r1, const urmapx_result *r2, const urmapx_path_op *path_ops,
                     const char *label1, const uint8_t *seq1, const uint8_t *qual1, uint32_t len1, const char *label2,
                     const uint8_t *seq2, const uint8_t *qual2, uint32_t len2, char *buf, size_t cap);

/* ---- Optional fields (-tags NM,MD,AS and -rg): SAM specification section 1.5, SAMtags ----
 * Behind QUAL, in this order whatever order they were asked for in: NM:i, MD:Z, AS:i, RG:Z.  An unmapped record (RNAME '*') gets RG only.
 * The alignment columns of a mapped record are what the record itself shows: POS, the CIGAR as emitted (after the dangling-M polish; it
 * may begin or end with an I or D run) and SEQ as printed (reverse-complemented for a minus-strand hit), against the bytes of the
 * sequence store from that sequence's offset + POS - 1 on.  Two letters match when their 4-bit BAM codes ("=ACMGRSVTWYHKDBN", either
 * case, anything else 15) are equal and not 15, which is samtools calmd's test: case never matters, N against N is a mismatch, R against
 * R a match.  NM = mismatching columns of M runs + bases of I runs + bases of D runs.  MD = [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*: a running
 * count of matches; at a mismatch the count, the reference letter in upper case, count = 0; at a D run the count, '^', the deleted
 * reference letters in upper case, count = 0; an I run neither prints nor resets; the final count always ("^AC0T" and a leading 0
 * occur).  AS = urmapx_result.score of the hit the record reports.  RG = the ID of the read-group line.
 * In BAM the same fields in the same order as aux fields: NM and AS in the smallest of C S I (value >= 0) or c s i (value < 0) that holds
 * the value, as htslib picks; MD and RG as Z with their NUL; block_size covers them; bin and what -sort derives from a record do not change. */
#define URMAPX_TAG_NM 1u
#define URMAPX_TAG_MD 2u
#define URMAPX_TAG_AS 4u
#define URMAPX_TAG_ALL 7u
/* What the tagged formatters take: tags = URMAPX_TAG_* bits; rg_id = the read group's ID or NULL (no RG field); ref[m] = the bytes of the
 * sequence store under mate m's record (single-end: ref[0]), from its first reference base on and as long as the reference bases its
 * CIGAR spans (urmapx_ref_span), or NULL: they are read from the index's host arrays (an index without them: the record is refused, 0). */
typedef struct urmapx_tag_options {
	unsigned tags;
	const char *rg_id;
	const uint8_t *ref[2];
} urmapx_tag_options;
/* NM and MD of one alignment by the rules above, no device and no index: ref = the reference window (ref_len bytes from the record's first
 * reference base), cigar[n_cigar] = the emitted runs as BAM packs them (len << 4 | op, op 0 M, 1 I, 2 D), seq = SEQ as printed.  Returns
 * the length of the MD text and writes it (no NUL) if it fits md_cap (md may be NULL to ask); *nm receives NM.  (size_t)-1: the runs
 * leave seq[seq_len] or ref[ref_len], or an op is none of the three. */
size_t urmapx_calmd(const uint8_t *ref, size_t ref_len, const uint32_t *cigar, uint32_t n_cigar, const uint8_t *seq, size_t seq_len,
                    uint32_t *nm, char *md, size_t md_cap);
/* reference bases under a result's emitted CIGAR (M and D runs; read_len for a result without a path); 0 for an unmapped result */
uint32_t urmapx_ref_span(const urmapx_result *r, const urmapx_path_op *path_ops, uint32_t read_len);
/* urmapx_sam_se / _pe / urmapx_bam_se / _pe with optional fields.  tags NULL: the bytes of the functions without _tags. */
size_t urmapx_sam_se_tags(const urmapx_index *, const urmapx_result *r, const urmapx_path_op *path_ops, const char *label,
                          const uint8_t *seq, const uint8_t *qual, uint32_t read_len, const urmapx_tag_options *tags, char *buf, size_t cap);
size_t urmapx_sam_pe_tags(const urmapx_index *, const urmapx_result *r1, const urmapx_result *r2, const urmapx_path_op *path_ops,
                          const char *label1, const uint8_t *seq1, const uint8_t *qual1, uint32_t len1, const char *label2,
                          const uint8_t *seq2, const uint8_t *qual2, uint32_t len2, const urmapx_tag_options *tags, char *buf, size_t cap);
size_t urmapx_bam_se_tags(const urmapx_index *, const urmapx_result *r, const urmapx_path_op *path_ops, const char *label,
                          const uint8_t *seq, const uint8_t *qual, uint32_t read_len, const urmapx_tag_options *tags, char *buf, size_t cap);
size_t urmapx_bam_pe_tags(const urmapx_index *, const urmapx_result *r1, const urmapx_result *r2, const urmapx_path_op *path_ops,
                          const char *label1, const uint8_t *seq1, const uint8_t *qual1, uint32_t len1, const char *label2,
                          const uint8_t *seq2, const uint8_t *qual2, uint32_t len2, const urmapx_tag_options *tags, char *buf, size_t cap);
/* A read-group line as `bwa mem -R` takes it: "@RG" then fields separated by real tabs or by the two characters '\' 't'.  Writes the
 * line with real tabs to line_out and the value of its ID: field to id_out (both NUL terminated; either may be NULL) and returns
 * URMAPX_OK, or URMAPX_E_ARG with the reason in err: the line does not start with "@RG" and a tab, has no ID: field, an empty ID, or a
 * newline. */
int urmapx_read_group_id(const char *line, char *line_out, size_t line_cap, char *id_out, size_t id_cap, char *err, size_t errcap);
/* The header text (@SQ lines, @PG with cmdline) and the BAM header block with a read-group line (tabs real, no '\n'; NULL: none)
 * directly in front of the @PG line; sorted != 0: "@HD\tVN:1.6\tSO:coordinate" first, as -sort writes it.  Return the size and write
 * it if it fits cap (buf may be NULL to ask). */
size_t urmapx_sam_header_rg(const urmapx_index *, const char *cmdline, const char *read_group, int sorted, char *buf, size_t cap);
size_t urmapx_bam_header_rg(const urmapx_index *, const char *cmdline, const char *read_group, int sorted, void *buf, size_t cap);
/* The bytes of the sequence store under n spans (starts[i] = offset in the store, lens[i] bytes) back to back into out, which holds
 * the sum of lens.  From the host arrays where the index has them; otherwise (urmapx_index_open_device) one gather on the index's
 * device and one copy for the whole list.  URMAPX_E_ARG: a span that leaves the store, or an index with neither. */
int urmapx_index_fetch_spans(const urmapx_index *, const uint64_t *starts, const uint32_t *lens, uint32_t n, uint8_t *out);
/* The device text stage with optional fields: mask = URMAPX_TAG_* bits, rg_id = the read group's ID or NULL (copied).  The chunk's
 * records then carry the fields, written by the two kernels of tags_gpu.hip around the record kernels; 0 and NULL: the records end at
 * QUAL again.  URMAPX_E_ARG while a chunk is in flight or waiting to be fetched, and for bits outside URMAPX_TAG_ALL. */
int urmapx_text_set_tags(urmapx_text *, unsigned mask, const char *rg_id);
/* Device time (ms, events) of the two tag passes of the last chunk whose text was made: [0] the pass that counts, [1] the pass that
 * writes; both 0 without tags. */
int urmapx_text_tag_ms(urmapx_text *, float ms[2]);
/* Stage-level entry point (the device functions the text stage runs; synchronous on the context's stream).  Host arrays: reads as
 * urmapx_map_se takes them, results[n] and the path arena as it returns them, mask = URMAPX_TAG_* bits.  Per record: nm[i], tagged[i] = 1
 * if the record gets NM / MD / AS (it is mapped), and its MD text at md + md_offs[i] .. md_offs[i + 1] (md_offs[n + 1]; an untagged
 * record's is empty).  *md_used receives md_offs[n]; with md_cap smaller nothing is written to md (URMAPX_E_ARG, *md_used still set).
 * URMAPX_E_ARG also for a result whose alignment leaves its read or its sequence. */
int urmapx_tags_batch(urmapx_ctx *, const uint8_t *bases, const uint64_t *offs, uint32_t n, const urmapx_result *results,
                      const urmapx_path_op *path_ops, size_t path_n, unsigned mask, uint32_t *nm, uint8_t *tagged, char *md, size_t md_cap,
                      uint64_t *md_offs, size_t *md_used);

/* ---- Sorted BAM output (-bamout ... -sort): coordinate order and a .bai index (SAM/BAM specification v1, section 5.2) ----
 * records[n_bytes]: BAM alignment records back to back on the host, each led by its block_size, as urmapx_text_set_bam, urmapx_bam_se
 * and urmapx_bam_pe make them.  A record's key is what it carries: refID read as unsigned (-1 sorts behind every reference), then pos
 * read as unsigned, then its place in the input (the sort is stable).  The result:
 *   bgzf / bgzf_bytes   the sorted records as BGZF members, cut every 65 280 bytes counted from the first byte of the first record:
 *                       no header block in front, no end-of-file member behind
 *   stream_bytes        the bytes those members inflate to (= n_bytes)
 *   bai / bai_bytes     the index file of a BAM file that holds bytes_in_front bytes (its compressed header block), then these members,
 *                       then the end-of-file member.  A place u of the sorted stream is written as the virtual offset
 *                       (file offset of member u / 65280) << 16 | u % 65280; the end of the stream, where it falls on a cut, points at
 *                       the end-of-file member.  Per reference: the bins present in ascending order, each with its chunks -- maximal runs
 *                       of records that follow one another in the file and share the bin (reg2bin of pos and pos + the reference bases
 *                       of the CIGAR, at least one) --, then the pseudo-bin 37450 (where the reference's records begin and end; how many
 *                       there are without and with flag 4), then the linear index: for every 16 384-base window the smallest place of
 *                       a record that overlaps it, a window without one taking the next one's value, cut off behind the last window
 *                       that has one.  n_no_coor counts the records with refID -1.  The scheme covers positions below 2^29 of a
 *                       reference.  A record with pos >= 2^29 is sorted like the others and counted in its reference's pseudo-bin,
 *                       between whose offsets it lies, but gets no chunk and no window.  A record that begins below 2^29 and ends
 *                       beyond is indexed as [pos, 2^29): that region's bin, the windows pos >> 14 .. 32 767.  So no bin but the
 *                       pseudo-bin exceeds 37 448, no linear index has more than 32 768 entries, and the index is well formed and
 *                       answers every region below 2^29 whatever lies beyond.  The record's own bin field stays what it carries.
 * Both byte arrays are the result's until urmapx_bam_sort_free.  The times are seconds of the calling thread in the steps named.
 * urmapx_bam_sort runs on `device` (bam_sort.hip): the record starts come from one walk along the block_size chain on the host, which
 * also checks the chain; keys, a least-significant-digit radix sort of (key, record number) in 8-bit digits over as many digits as n_ref
 * and the largest pos need, the gather of the records into sorted order, the index arrays and the deflate are kernels.  The sorted
 * stream is made, compressed and copied back in slices of a multiple of 65 280 bytes (URMAPX_TEST_SORT_SLICE=N: of N members), so the
 * device holds the unsorted records, the per-record arrays (urmapx_bam_sort_device_bytes says how much in all) and one slice.
 * urmapx_bam_sort_external lifts "the records must fit": it plans from a budget of device bytes (urmapx_bam_sort_plan_for) and takes
 * the road the plan names.  In core: the call above.  External: only the per-record arrays stay on the device -- 48 bytes a record,
 * under marking 25 more -- and the records stream through two staging buffers in input order, 1 + P times: once for the keys, the ends,
 * the flag-4 bits and what the marking reads, then once per partition of the sorted stream (P partitions, each a whole number of
 * slices), where place_kernel copies the part of every staged record that falls into the partition to its place and sets or clears
 * bit 0x400 on the way.  A filled partition is deflated slice by slice as in core, so the members, the stream and the index are the
 * in-core call's.  budget_bytes 0: what hipMemGetInfo reports free less URMAPX_SORT_HEADROOM.  md NULL: no marking.  The per-record
 * arrays must still fit the device, the result still lies in host memory.  URMAPX_TEST_SORT_PARTITION=N: external with partitions of N
 * slices whatever the budget; URMAPX_TEST_SORT_STAGE=B: staged chunks of B bytes (whole records, one at the least).
 * urmapx_bam_sort_host: the same contract by std::stable_sort, plain loops and urmapx_bgzf_compress_host; no device.  The two give the
 * same inflated stream and, expressed in places of the stream, the same index; their compressed bytes differ.
 * starts[n_starts] (optional, NULL / 0: none): offsets in `records`, ascending, at which the caller knows a record to begin (the pieces
 * it put the array together from).  The walk along the chain -- one pass over all the bytes at one thread's pace otherwise -- then runs
 * from all of them at once, each up to the next, which it must hit exactly (URMAPX_E_FORMAT if not).
 * URMAPX_E_FORMAT: the bytes are no chain of records (a block_size that runs past the end or does not hold its own name and CIGAR, a
 * refID outside -1 .. n_ref - 1, a pos below -1, a refID without a pos); URMAPX_E_NOMEM; URMAPX_E_NODEVICE. */
typedef struct urmapx_bam_sort_result {
	void *bgzf, *bai;
	size_t bgzf_bytes, bai_bytes;
	uint64_t stream_bytes, records, no_coor;
	uint32_t sort_passes;    /* histogram-scan-scatter rounds of the coordinate sort (device) */
	uint32_t slices;         /* pieces the sorted stream was made in (device) */
	double scan_s;           /* the walk along the block_size chain (host, both versions) */
	double alloc_s;          /* device: hipMalloc and hipFree of the call's arrays.  Inside no other part, but for the arrays that are
	                          * allocated once their sizes are known: the linear index and the chunks (also inside index_s) and, in
	                          * core, the marking's own (also inside markdup_s) */
	double upload_s, sort_s, gather_s, deflate_s, copy_s, index_s;  /* records to the device; key + sort launches; gather launches; the
	                          * compressor; members back to the host; index kernels and the .bai bytes.  Host version: sort_s (the sort),
	                          * gather_s (the copy into order), deflate_s, index_s */
	uint32_t external;       /* 1: the records were streamed through the device (urmapx_bam_sort_external's external road) */
	uint32_t partitions;     /* external: pieces of the sorted stream that were filled one after the other; 0 in core */
	uint64_t stage_chunks;   /* external: staged chunks of one pass over the input */
	double stage_s;          /* external: the 1 + partitions passes over the input -- copies to the staging buffers, keys_kernel and the
	                          * marking's record kernels in the first, place_kernel in the others (upload_s: the record starts alone;
	                          * gather_s: 0) */
} urmapx_bam_sort_result;
int urmapx_bam_sort(int device, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                    size_t n_starts, urmapx_bam_sort_result *out);
int urmapx_bam_sort_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts, size_t n_starts,
                         urmapx_bam_sort_result *out);
void urmapx_bam_sort_free(urmapx_bam_sort_result *);
/* device memory urmapx_bam_sort takes for n_bytes of records in n_records records (slice and compressor scratch included) */
uint64_t urmapx_bam_sort_device_bytes(size_t n_bytes, uint64_t n_records);
/* The road urmapx_bam_sort_external takes for a budget of device bytes (host arithmetic).  In core (external 0; device_bytes =
 * urmapx_bam_sort[_markdup]_device_bytes, the other fields 0) when that fits the budget.  Otherwise external: staged chunks of stage_bytes
 * (a tuning value, n_bytes / 16 at the most), partitions of partition_bytes -- the largest whole number of slices with which
 * device_bytes, the sum the allocations follow, stays within the budget -- and partitions = ceil(n_bytes / partition_bytes).
 * URMAPX_E_NOMEM when even one slice does not fit: device_bytes is then the least budget that does. */
typedef struct urmapx_bam_sort_plan {
	int external;            /* 0: the in-core road */
	uint64_t partition_bytes, partitions, stage_bytes, device_bytes;
} urmapx_bam_sort_plan;
int urmapx_bam_sort_plan_for(size_t n_bytes, uint64_t n_records, int markdup, uint64_t budget_bytes, urmapx_bam_sort_plan *plan);
#define URMAPX_SORT_HEADROOM ((uint64_t)256 << 20)  /* device bytes left alone when the budget is taken from hipMemGetInfo */
/* (urmapx_bam_sort_external itself is declared behind urmapx_markdup_stats, below) */

/* ---- Duplicate marking (-bamout ... -sort -markdup): flag 0x400, decided while the records lie on the device for the sort ----
 * urmapx_bam_sort_markdup / _host: urmapx_bam_sort / _host with one step more.  Order, cuts and index are those of the plain call;
 * only bit 0x400 of the records' flag half-words may differ.  The rule is Picard's and samtools', without libraries and without
 * optical duplicates.  The input is the records in input order; all arithmetic on positions is signed and 64 bits wide.
 *  1. Eligible: a record with none of the flags 0x4, 0x100, 0x800.  Every other record is copied untouched, with whatever 0x400 it
 *     carries.  An eligible record's 0x400 on output is set exactly when the rules below make it a duplicate (an incoming 0x400 is
 *     overwritten).
 *  2. The end of a record: E = (refID, u5, rev).  rev is flag 0x10.  Forward: u5 = pos - (the S and H lengths in front of the first
 *     reference-consuming op).  Reverse: u5 = pos + refspan - 1 + (the S and H lengths behind the last reference-consuming op).
 *     refspan is the sum over M, D, N, =, X (not cut off at 2^31), 1 for a record without such an op; for that record every S and H op
 *     counts as in front and as behind.  u5 may be negative.  Ends are ordered by refID (as unsigned), then u5 (signed), then rev.
 *  3. Pair: records i and i + 1 of the input, both eligible, i with flags 0x1 and 0x40 and without 0x80, i + 1 with 0x1 and 0x80, their
 *     read_names equal byte for byte (equal l_read_name included).  A record is in at most one pair: scanning from the front, a record
 *     taken as a second mate is not tried as a first mate.  Every other eligible record is a fragment: single-end reads, mates whose
 *     partner is unmapped, mates that are not adjacent.
 *  4. Score of a record: the sum of its QUAL bytes q with 15 <= q and q != 0xFF, at most 2^31 - 1 (it saturates there: over eight
 *     million bases).  Score of a pair: the sum over its two records.
 *  5. Pairs: the key of a pair is (min(E1, E2), max(E1, E2)).  Among the pairs of one key the one with the largest score stays, ties
 *     going to the pair whose first record comes first in the input; both records of every other pair are duplicates.
 *  6. Fragments: all eligible records grouped by E, members of pairs included.  If the group holds a member of a pair, every fragment
 *     in it is a duplicate; otherwise the fragment with the largest score stays (ties: first in the input) and the others are
 *     duplicates.  Members of pairs are decided by rule 5 alone.
 *  7. pairs_examined counts pairs, pairs_duplicate flagged pairs (not records), fragments_examined fragments, fragments_duplicate
 *     flagged fragments.
 * The result is a function of the records in input order.  The device version (markdup.hip) and the host version (markdup_host.cpp,
 * written apart from it: std::stable_sort on a tuple and a walk over the groups) give the same inflated stream and counters.
 * URMAPX_E_FORMAT in addition to urmapx_bam_sort's: an eligible record whose SEQ and QUAL (l_seq) do not lie inside its block_size;
 * device version only: ends whose packed form -- bits for n_ref, for the span of u5 seen, one for rev -- exceeds 64 bits (more
 * references and longer clips than any file has). */
typedef struct urmapx_markdup_stats {
	uint64_t pairs_examined, pairs_duplicate, fragments_examined, fragments_duplicate;
	double markdup_s;        /* seconds of the calling thread in the marking (device: its launches and copies; inside no part of the result's times) */
} urmapx_markdup_stats;
int urmapx_bam_sort_markdup(int device, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                            size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out);
int urmapx_bam_sort_markdup_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                                 size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out);
/* device memory urmapx_bam_sort_markdup takes: urmapx_bam_sort_device_bytes and 24 bytes a record for ends, best words and roles
 * (urmapx_bam_sort_external with md on its external road: 25 a record, the record bytes not among them) */
uint64_t urmapx_bam_sort_markdup_device_bytes(size_t n_bytes, uint64_t n_records);
/* the planned sort ("Sorted BAM output" above): in core or streamed, as urmapx_bam_sort_plan_for says for budget_bytes; md NULL: no marking */
int urmapx_bam_sort_external(int device, uint64_t budget_bytes, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front,
                             const uint64_t *starts, size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out);

/* ---- Depth (per-base coverage of BAM records, as a bedGraph text and a summary per reference) ----
 * The input is BAM records as above, in any order, n_ref reference names (C strings of 1 .. 255 bytes: the names of the @SQ lines) and
 * their lengths l_ref.  The rule is `samtools depth` without -J, -s and base-quality filters; the result is exact.
 *  1. Eligible: a record with 0 <= refID < n_ref, pos >= 0, (flag & 0x704) == 0 -- not unmapped, secondary, QC-fail or duplicate -- and
 *     MAPQ >= min_mapq.  The flag is the one the record carries; inside urmapx_bam_sort_with it is the one the record carries in the
 *     sorted stream, so under marking bit 0x400 is the marking's decision, not the incoming bit.  Supplementary records (0x800) count.
 *  2. Covered columns: the CIGAR is walked with a reference cursor c that starts at pos.  M, = and X of length L cover the columns
 *     [c, c + L) that lie in [0, l_ref) and advance c by L; D and N advance c and cover nothing; I, S, H and P do nothing.  Columns
 *     beyond the reference's length are dropped, which is no error.  Overlapping mates count twice.  A record without a CIGAR covers
 *     nothing (one whose CIGAR does not lie inside its block_size is refused with the chain: URMAPX_E_FORMAT).
 *  3. d(r, x), the depth of column x of reference r, is the number of covering ops.  All arithmetic on positions is 64 bits wide: the
 *     concatenated space of the counters, the sum over the references of l_ref + 1, may exceed 2^32.  The counters are 32 bits wide: a
 *     call with 2^31 records or more is URMAPX_E_ARG.
 *  4. Text: for every reference with l_ref > 0, in index order, [0, l_ref) is cut into maximal runs of equal depth and each run is one
 *     line "name\tbeg\tend\tdepth\n", 0-based and half-open, the numbers in decimal.  Runs of depth 0 are lines too, so the lines of a
 *     reference tile it exactly; a reference without reads is the one line "name\t0\tl_ref\t0".  No header line.
 *  5. Summary per reference: reads = the eligible records on it, whatever they cover; covered = its columns with d >= 1; bases = the
 *     sum of d over its columns; mapq_sum = the sum of MAPQ over its eligible records.
 * urmapx_bam_depth runs on `device` (depth.hip): the records pass through two staging buffers in input order (chunks of whole records,
 * URMAPX_TEST_SORT_STAGE=B: of B bytes), so its memory does not grow with n_bytes; depth_count_kernel adds +1 and -1 into a difference
 * array in which reference r owns l_ref + 1 entries -- an end that was clipped lands in the extra one, so every reference's entries
 * sum to zero and one inclusive scan of the whole array gives every reference's depths --, the runs are found and compacted a segment
 * of the array at a time, and their lines are made in slices of 65 536 runs (URMAPX_TEST_DEPTH_SLICE=N: of N) that are copied back
 * while the next one is formatted.  urmapx_bam_depth_host (depth_host.cpp, written apart from it: a difference array and a running
 * sum in plain loops) gives the same bytes and numbers.  starts / n_starts: as for the sort.
 * urmapx_bam_sort_with ("The planned sort with what is taken on the way" below) takes the depth while the records are on the device
 * for the sort: in core by one launch over the unsorted records once the marking has decided, on the external road on the chunks of
 * the first placing pass, where the marking's decisions lie complete beside the records.  The depth arrays
 * (urmapx_bam_depth_resident_bytes) come off the budget before the sort is planned; a budget that does not hold them is
 * URMAPX_E_NOMEM, and depth->least_budget then names the least budget that does.  urmapx_bam_sort_with_host: the host sort (with
 * marking when md is given) and urmapx_bam_depth_host of its stream.
 * URMAPX_E_ARG: a name that is empty or longer than 255 bytes, 2^31 records or more; else the sort's codes. */
typedef struct urmapx_depth_opts {
	uint32_t min_mapq;
} urmapx_depth_opts;
typedef struct urmapx_depth_summary {
	uint64_t reads, covered, bases, mapq_sum;
} urmapx_depth_summary;
typedef struct urmapx_depth_result {
	char *text;              /* the bedGraph lines (malloc; not terminated) */
	size_t text_bytes;
	uint64_t runs;           /* lines of the text */
	urmapx_depth_summary *refs;  /* n_ref of them */
	uint32_t n_ref;
	uint32_t text_slices;    /* device: pieces the text was formatted and copied back in */
	uint64_t records;        /* records seen, eligible or not */
	uint64_t stage_chunks;   /* urmapx_bam_depth: staged chunks of its pass over the input */
	uint64_t least_budget;   /* urmapx_bam_sort_with under URMAPX_E_NOMEM from the budget: the least budget_bytes that holds the call */
	double alloc_s, count_s, scan_s, runs_s, format_s, copy_s;  /* device arrays; staging and depth_count_kernel (host: the CIGAR walk);
	                          * the scan (host: the running sum and the runs); boundary flags, compaction and the summaries; the lines;
	                          * the lines back to the host (inside no other part) */
} urmapx_depth_result;
int urmapx_bam_depth(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                     const uint64_t *starts, size_t n_starts, const urmapx_depth_opts *opts, urmapx_depth_result *out);
int urmapx_bam_depth_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                          const uint64_t *starts, size_t n_starts, const urmapx_depth_opts *opts, urmapx_depth_result *out);
void urmapx_depth_free(urmapx_depth_result *);
/* device memory urmapx_bam_depth takes for references of total_columns columns in all and n_records records, with staged chunks of
 * the default size (the sum its allocations follow: depth.h) */
uint64_t urmapx_bam_depth_device_bytes(uint64_t total_columns, uint32_t n_ref, uint64_t n_records);
/* what of that the depth adds to urmapx_bam_sort_with: no staging buffers and no record starts of its own */
uint64_t urmapx_bam_depth_resident_bytes(uint64_t total_columns, uint32_t n_ref);

/* ---- Stats (alignment QC tables of BAM records, as a tab-separated text) ----
 * The input is BAM records as above, in any order, and the n_ref reference names and lengths (as for the depth).  Every counter is 64
 * bits wide and exact, and no counter depends on the order of the records.
 *  1. Flags are the ones the record carries; inside urmapx_bam_sort_with they are the ones it carries in the sorted stream, so under
 *     marking bit 0x400 is the marking's decision.  A READ is a record with neither 0x100 nor 0x800.  The counters records, secondary
 *     (0x100) and supplementary (0x800) count records; everything else counts reads only.  MAPPED: not 0x4.  LAST FRAGMENT: 0x80 set;
 *     every other read is a FIRST FRAGMENT.
 *  2. Fields.  l_seq, CIGAR, SEQ, QUAL and the aux area (from the end of QUAL to the end of block_size) are the record's.  A read whose
 *     SEQ and QUAL do not lie inside its block_size counts with l_seq 0, no CIGAR op and no aux area.
 *  3. Caps: CYCLES 1024, QUALS 94, IS_MAX 8000, RL_MAX 65535, ID_MAX 256; a value beyond a cap falls into the last bin (min(v, cap)).
 *     Cycle of base i (0-based) of a read of l_seq bases: i, or l_seq - 1 - i where 0x10 is set.  Cycles >= CYCLES share one extra row.
 *     Base classes from the 4-bit codes: A=1, C=2, G=4, T=8, N=15, every other code "other"; where 0x10 is set A<->T and C<->G swap.
 *     A read HAS QUALITIES if l_seq > 0 and its first QUAL byte is not 0xFF; a quality value is min(QUAL byte, 93).
 *  4. CIGAR sums, over mapped reads: bases mapped (cigar) = lengths of M, =, X, I; bases soft clipped = S; bases inserted = I; bases
 *     deleted = D; insertions / deletions = the I / D ops of length >= 1.  ID bin of such an op: min(length, ID_MAX).
 *  5. NM.  The aux area of a mapped read is walked field by field: tag (2 bytes), type (1), value -- A c C: 1 byte; s S: 2; i I f: 4;
 *     Z H: up to and including a 0 byte; B: a subtype of c C s S i I f, a 32-bit count, count elements.  A field that would leave
 *     block_size, an unknown type or subtype, or fewer than 3 bytes left end the walk.  The first field met with tag NM and a type of
 *     c C s S i I gives the read's NM (signed for c s i; negative counts as 0) and ends the walk; the read is then a READ WITH NM.  An NM
 *     field of another type is walked over.  mismatches = the sum of NM; error rate = mismatches / (the M, =, X, I lengths of the reads
 *     with NM), six decimals.
 *  6. Insert size.  A read contributes when 0x1 is set, it is mapped, 0x8 is not set, next_refID == refID and tlen > 0: one record per
 *     pair, judged from the record alone.  Inward: 0x10 clear and 0x20 set.  Outward: 0x10 set and 0x20 clear.  Else "other".  The size
 *     is min(tlen, IS_MAX).  insert size average: over the binned sizes, two decimals.  insert size median: the least size whose
 *     cumulative count reaches ceil(pairs / 2); 0 without pairs.
 *  7. Quotients: floor((10^d * num + den / 2) / den) in integers (den / 2 rounded down), printed with the point in front of the last d
 *     digits; "0." and d zeros where den is 0.
 *  8. The text: lines of tab-separated fields, each led by its section tag, in this order.
 *       "# urmapx stats 1"  and  "# command: " followed by the command text (the @PG command of the run; empty for library calls)
 *       SN <name> <value>, one line each, in this order: records; secondary; supplementary; reads; reads paired (0x1); first fragments;
 *          last fragments; reads mapped; reads unmapped; reads properly paired (0x1, 0x2, mapped); reads mapped and paired (0x1, mapped,
 *          not 0x8); singletons (0x1, mapped, 0x8); mate on another reference (mapped and paired, next_refID != refID); reads reverse
 *          strand (mapped, 0x10); reads duplicated (0x400); reads QC failed (0x200); reads MQ0 (mapped, MAPQ 0); reads without qualities
 *          (l_seq > 0, first QUAL byte 0xFF); total length (sum of l_seq); bases mapped (l_seq of mapped reads); bases mapped (cigar);
 *          bases soft clipped; bases inserted; bases deleted; insertions; deletions; bases duplicated (l_seq of reads with 0x400); reads
 *          with NM; mismatches; error rate; average length (total length / reads, two decimals); maximum length (of l_seq); average
 *          quality (the quality values of the reads with qualities / their bases, two decimals); pairs with insert size; inward pairs;
 *          outward pairs; other pairs; insert size average; insert size median
 *       RL length first last      reads by min(l_seq, RL_MAX), first and last fragments; lengths with a count only
 *       MQ mapq count             mapped reads; rows with a count only
 *       IS size total inward outward other    rows with a count only
 *       FFQ / LFQ cycle c0 .. c93 first / last fragments with qualities: per cycle (printed 1-based) the reads with each quality value;
 *                                 rows 1 .. the largest cycle below CYCLES with a count in that table, then a row ">1024" if it has one
 *       BC cycle A C G T N other  all reads; rows as for FFQ
 *       GC percent count          reads with l_seq > 0 by floor(100 * (#C + #G) / l_seq), codes 2 and 4; rows with a count only
 *       ID length insertions deletions        rows with a count only
 *       RF name length mapped unmapped duplicated   reads by refID, one line per reference in index order, zeros included; a last
 *                                 line with name "*" and length 0 for refID -1
 * urmapx_bam_stats runs on `device` (stats.hip): the records pass through two staging buffers in input order, as for the depth
 * (URMAPX_TEST_SORT_STAGE=B), and stats_count_kernel -- persistent workgroups, a wavefront per record, the hot low ends of the tables
 * in LDS, added to the 64-bit tables once per workgroup and launch (URMAPX_TEST_STATS_BLOCKS=N: at most N workgroups) -- counts them;
 * the tables (urmapx_bam_stats_resident_bytes) are copied back and one host formatter writes the text.  urmapx_bam_stats_host
 * (stats_host.cpp): a plain loop on one thread and the same formatter; the same bytes.  starts / n_starts: as for the sort.  command:
 * the text of the second line, NULL: empty.
 * URMAPX_E_ARG: a name that is empty or longer than 255 bytes, 2^31 records or more; else the sort's codes. */
typedef struct urmapx_stats_result {
	char *text;              /* the text (malloc; not terminated) */
	size_t text_bytes;
	uint64_t records, reads, mapped, properly_paired, duplicated, insert_median;  /* the SN lines of those names */
	uint64_t stage_chunks;   /* urmapx_bam_stats: staged chunks of its pass over the input */
	uint64_t least_budget;   /* urmapx_bam_sort_with under URMAPX_E_NOMEM from the budget: the least budget_bytes that holds the call */
	double alloc_s, count_s, format_s;  /* device tables; staging and stats_count_kernel (host: the loop); tables back and the text */
} urmapx_stats_result;
int urmapx_bam_stats(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                     const uint64_t *starts, size_t n_starts, const char *command, urmapx_stats_result *out);
int urmapx_bam_stats_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                          const uint64_t *starts, size_t n_starts, const char *command, urmapx_stats_result *out);
void urmapx_stats_free(urmapx_stats_result *);
/* device bytes of the statistics' tables: what they add to the planned sort (the sum the allocation follows: stats.h) */
uint64_t urmapx_bam_stats_resident_bytes(uint32_t n_ref);

/* ---- Pileup (SNV candidate sites of BAM records against the reference bases, as a sites-only VCF 4.2 text) ----
 * The input is BAM records as above, in any order, the n_ref reference names and lengths (as for the depth) and the reference bases,
 * lens[r] ASCII letters per reference.  Every rule is exact integer arithmetic and no count depends on the order of the records.
 *  1. Which records count: exactly the depth's (items 1-2 of "Depth").  The record has a reference (0 <= refID < n_ref) and a position
 *     (pos >= 0), none of the flags 0x704 as the file carries them -- inside urmapx_bam_sort_with under marking bit 0x400 is the
 *     marking's decision, not the incoming bit (on the external road the action byte stands in) --, and its MAPQ is at least min_mapq
 *     (default 0).  Supplementary records (0x800) count.  A record whose CIGAR, SEQ and QUAL do not lie inside its block_size counts
 *     as a record and adds no base.
 *  2. Which bases count.  The walk over the CIGAR keeps a query cursor (from 0) and a reference cursor (from pos).  M, = and X cover:
 *     query base q lies on column x, and both cursors advance.  I and S advance the query cursor, D and N the reference cursor, H, P
 *     and the unused op codes neither.  A base counts when its column is below l_ref, its query offset is below l_seq, its 4-bit code
 *     is 1, 2, 4 or 8 (A, C, G, T) and its quality is at least min_baseq (default 13).  Every other code (N, IUPAC, =) counts nowhere.
 *     A record with l_seq > 0 whose first QUAL byte is 0xFF has no qualities: all its bases pass.  Overlapping mates count twice, as
 *     in the depth.
 *  3. Per column: four counters cnt[A], cnt[C], cnt[G], cnt[T]; DP is their sum.  The reference letter is the sequence's byte, case
 *     folded.  A column whose reference letter is not one of A C G T is never a site.  A base b other than the reference's is an
 *     alternative allele when cnt[b] >= min_alt (default 3; at least 1) and cnt[b] * 100 >= min_pct * DP (min_pct 0 .. 100, default
 *     10), both in 64-bit integers.  A column with at least one alternative allele is a site.
 *  4. The text.  The header: "##fileformat=VCFv4.2", "##source=urmap", "##urmapCommand=" followed by the command text (empty for NULL),
 *     one "##contig=<ID=name,length=l_ref>" per reference in index order,
 *     "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Bases counted on the column\">",
 *     "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Bases counted per allele, the reference's first\">" and
 *     "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO".  Then one line per site, by reference in index order, then by position:
 *       name \t pos+1 \t . \t REF \t ALT[,ALT..] \t . \t . \t DP=n;AD=ref,alt1[,alt2..]
 *     REF is the folded letter; the alternative alleles stand by count descending, ties in the order A, C, G, T; numbers are decimal.
 * Limits: the counters are uint32; 2^31 records or more are URMAPX_E_ARG, so none wraps.  All column arithmetic is 64 bits wide.
 * The defaults are choices, not measurements: 13 is samtools mpileup's base-quality floor; 3 reads and 10 % keep single sequencing
 * errors out at 30-fold coverage.  With min_baseq 0 and reads without N a site's DP is the depth of its column for the same MAPQ floor.
 *
 * urmapx_bam_pileup runs on `device` (pileup.hip): the sequences are uploaded (a byte a base), the records pass through two staging
 * buffers in input order (URMAPX_TEST_SORT_STAGE=B) and pileup_count_kernel -- a persistent grid, a wavefront per record, the CIGAR 64
 * ops a step, the covered bases 64 a step with one atomic add a lane (URMAPX_TEST_PILEUP_BLOCKS=N: at most N workgroups) -- counts
 * them into one 16-byte entry per reference column.  The sites are found a segment of columns at a time (URMAPX_TEST_PILEUP_SEGMENT=N
 * columns), compacted into entries of 24 bytes and copied back a slice at a time (URMAPX_TEST_PILEUP_SLICE=N entries) through two
 * page-locked buffers; one host formatter writes the text.  urmapx_bam_pileup_host (pileup_host.cpp): a plain walk on one thread and
 * the same formatter; the same bytes.  seqs[r]: lens[r] letters (may be NULL where lens[r] is 0).  opts NULL: the defaults.
 * URMAPX_E_ARG: a name that is empty or longer than 255 bytes, a missing sequence, min_mapq or min_baseq above 255, min_alt 0, min_pct
 * above 100, 2^31 records or more; else the sort's codes. */
typedef struct urmapx_pileup_opts {
	uint32_t min_mapq, min_baseq, min_alt, min_pct;
} urmapx_pileup_opts;
typedef struct urmapx_pileup_result {
	char *text;              /* the text (malloc; not terminated) */
	size_t text_bytes;
	uint64_t sites, alt_alleles, records;  /* lines behind the header; ALT entries over all lines; records that counted (rule 1) */
	uint64_t stage_chunks;   /* urmapx_bam_pileup: staged chunks of its pass over the input */
	uint64_t least_budget;   /* urmapx_bam_sort_with under URMAPX_E_NOMEM from the budget: the least budget_bytes that holds the call */
	double alloc_s, count_s, sites_s, format_s, copy_s;  /* device arrays; staging and pileup_count_kernel (host: the walk); the site
	                          * kernels (host: the scan of the columns); the text; waiting for the slices' copies */
} urmapx_pileup_result;
int urmapx_bam_pileup(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                      const uint8_t *const *seqs, const uint64_t *starts, size_t n_starts, const urmapx_pileup_opts *opts, const char *command,
                      urmapx_pileup_result *out);
int urmapx_bam_pileup_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                           const uint8_t *const *seqs, const uint64_t *starts, size_t n_starts, const urmapx_pileup_opts *opts,
                           const char *command, urmapx_pileup_result *out);
void urmapx_pileup_free(urmapx_pileup_result *);
/* device bytes of the pileup's arrays: what they add to the planned sort (the sum the allocation follows: pileup.h).  seq_resident
 * not 0: the reference bases are read in place (an index resident on the sort's device); 0: a byte a base more for their upload */
uint64_t urmapx_bam_pileup_resident_bytes(uint64_t total_columns, uint32_t n_ref, int seq_resident);
/* what urmapx_bam_pileup takes: those with the upload, the record starts and two staging buffers */
uint64_t urmapx_bam_pileup_device_bytes(uint64_t total_columns, uint32_t n_ref, uint64_t n_records);

/* ---- The planned sort with what is taken on the way ----
 * urmapx_bam_sort_external with the depth, the statistics and the pileup, each or none, taken while the records are on the device: in
 * core by their launches over the unsorted records once the marking has decided, on the external road on the chunks of the first
 * placing pass.  md NULL: no marking.  depth NULL: no depth (dopts unused).  stats NULL: no statistics (stats_command unused).  pileup
 * NULL: no pileup (popts, seqs, index and pileup_command unused).  names and lens: needed with any of the three.  With none this is
 * urmapx_bam_sort_external.  The pileup's reference bases: seqs (as for urmapx_bam_pileup), or, with seqs NULL, index: its sequence
 * store, read in place where it is resident on `device`, else fetched once through urmapx_index_fetch_spans and uploaded; its
 * sequence count and lengths must be n_ref and lens (URMAPX_E_ARG).  The arrays of what is asked for come off the budget before the
 * sort is planned; under URMAPX_E_NOMEM from the budget the least_budget of every result asked for names the least budget that holds
 * the call.  _host: the host sort (with marking when md is given) and the host versions on its records. */
typedef struct urmapx_bam_sort_extras {
	urmapx_markdup_stats *md;
	const urmapx_depth_opts *dopts;
	const char *const *names;
	const uint32_t *lens;
	urmapx_depth_result *depth;
	urmapx_stats_result *stats;
	const char *stats_command;
	const urmapx_pileup_opts *popts;
	const uint8_t *const *seqs;
	const urmapx_index *index;
	urmapx_pileup_result *pileup;
	const char *pileup_command;
} urmapx_bam_sort_extras;
int urmapx_bam_sort_with(int device, uint64_t budget_bytes, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front,
                         const uint64_t *starts, size_t n_starts, const urmapx_bam_sort_extras *extras, urmapx_bam_sort_result *out);
int urmapx_bam_sort_with_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                              size_t n_starts, const urmapx_bam_sort_extras *extras, urmapx_bam_sort_result *out);

const char *urmapx_strerror(int code);
/* "gfx950" etc. of the ctx's device; NULL without a device */
const char *urmapx_device_arch(urmapx_ctx *);

#ifdef __cplusplus
}
#endif
#endif
