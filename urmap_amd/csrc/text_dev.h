// text_dev.h -- what the record kernels of the text stage share: the chunk header, a record's view of the FASTQ bytes and of its
// mate (SetSAM2's fields), the merged CIGAR runs of a path.  Included by text_gpu.hip (SAM text) and bam_gpu.hip (BAM records); the
// two are translation units of their own so that neither changes how the other's kernels are compiled.
#ifndef URX_TEXT_DEV_H
#define URX_TEXT_DEV_H
#include "internal.h"

namespace urx {

struct TextHdr {  // device; [0] and [1]: the chunk of each file (n_lines, n_records, flags, max_len); [0] also the call's totals
	uint32_t n_lines, n_records, flags, max_len;
	uint32_t total_bases, sam_total, n_reads, pad1;  // n_reads: records of the batch (single-end: n_records; pairs: twice that)
	unsigned long long cnt[4];  // accept, reject, nohit, unsupported
};

struct SamArgs {
	const uint8_t *raw[2];       // the chunk of each file (single-end: [0] only)
	const uint32_t *ends[2];
	uint32_t paired;             // records 2i, 2i+1 = the mates of pair i, from raw[0] and raw[1]
	const urmapx_result *results;
	const urmapx_path_op *ops;
	const char *tnames;          // target labels back to back
	const uint32_t *tname_offs;  // seqCount + 1
	const uint8_t *comp;         // 256-byte complement table (alpha.cpp:3005)
	uint32_t seq_count;
	uint32_t minq;
	TextHdr *hdr;
	uint32_t *lens;              // PASS 0 out
	uint32_t *qn;                // PASS 0 out: QNAME bytes of every record (PASS 1 does not scan the labels again)
	const uint32_t *rec_offs;    // PASS 1 in
	char *sam;                   // PASS 1 out
};

// bam_gpu.hip: the two passes of the BAM record encoder on a stream, a SAM pass in each one's place (PASS 0 fills lens / qn and the
// counters as sam_len_kernel does, PASS 1 writes the records to A.sam at rec_offs)
void bam_len_launch(const SamArgs &A, hipStream_t st);
void bam_launch(const SamArgs &A, hipStream_t st);

// tags_gpu.hip: the optional fields NM MD AS RG of a chunk's records (include/urmapx.h, "Optional fields").  The record kernels do not
// know of them: PASS 0 (tag_len_launch, behind the record length kernel) counts every record's field bytes and gives the prefix sum
// slots[i] = lens[i] + tag_len[i] in place of lens[i]; PASS 1 (tag_write_launch, behind the record kernel) puts the fields where the
// record kernel left room -- over the '\n' of a SAM record and behind it, behind a BAM record, whose block_size it raises.
struct TagArgs {
	SamArgs A;
	const uint8_t *store;        // the index's sequence store on the device
	const uint32_t *seq_offs;    // offset of every sequence in it
	uint32_t store_size;
	uint32_t mask;               // URMAPX_TAG_* bits
	const char *rg_id;           // device copy of the read group's ID; null: no RG field
	uint32_t rg_len;
	uint32_t bam;
	uint32_t *nm, *md_len, *tag_len;  // PASS 0 out, PASS 1 in: per record
	uint32_t *slots;             // PASS 0 out: what the scan of the record offsets takes
};
void tag_len_launch(const TagArgs &G, hipStream_t st);
void tag_write_launch(const TagArgs &G, hipStream_t st);

}  // namespace urx

using namespace urx;

namespace {

constexpr int SAM_WAVES = 4;        // wavefronts per block of the record kernels
// an LDS array named by an LDS pointer (32 bit, ds_* instructions), as in dev_common.h
template <class T> using lds_ptr = __attribute__((address_space(3))) T *;
template <class T> __device__ __forceinline__ lds_ptr<T> to_lds(T *p) { return (lds_ptr<T>)p; }

__device__ __forceinline__ uint32_t line_start(const uint32_t *ends, uint32_t k) { return k ? ends[k - 1] + 1u : 0u; }

// SetSAM's arguments (setsam.cpp:73-74): single-end passes 0, "*", UINT32_MAX, 0 (output1.cpp:13); pairs what SetSAM2
// works out (output2.cpp:61-128)
struct MateFields {
	uint32_t flags;
	bool mate_mapped;
	uint32_t mate_seq_index, mate_coord;
	int tlen;
};

__device__ __forceinline__ uint32_t paired_flags(bool first, bool revcomp, bool mate_revcomp, bool mate_unmapped) {  // output2.cpp:18-36
	uint32_t f = first ? 0x41u : 0x81u;
	if (revcomp) f |= 0x10u;
	if (mate_unmapped) f |= 0x08u;
	else if (mate_revcomp) f |= 0x20u;
	return f;
}

// SetSAM2 (output2.cpp:61-128) for mate `second` of a pair with results r1, r2 and read lengths len1, len2
__device__ MateFields pair_fields(const urmapx_result &r1, const urmapx_result &r2, uint32_t len1, uint32_t len2, bool second) {
	const bool m1 = r1.dbpos != 0xFFFFFFFFu, m2 = r2.dbpos != 0xFFFFFFFFu;
	const bool plus1 = m1 && r1.plus, plus2 = m2 && r2.plus;
	const bool consistent = m1 && m2 && (plus1 != plus2);
	int tlen1 = 0, tlen2 = 0;
	bool proper = false;
	if (m1 && m2) {
		if (r1.coord <= r2.coord) {
			tlen1 = (int)(r2.coord + len2) - (int)r1.coord;
			if (tlen1 > 0 && tlen1 < 1000 && consistent) proper = true;
			if (tlen1 > 1000) tlen1 = 0;
			tlen2 = -tlen1;
		} else {
			tlen2 = (int)(r1.coord + len1) - (int)r2.coord;
			if (tlen2 > 0 && tlen2 < 1000 && consistent) proper = true;
			if (tlen2 > 1000) tlen2 = 0;
			tlen1 = -tlen2;
		}
	}
	const bool rc1 = m1 && !r1.plus, rc2 = m2 && !r2.plus;
	MateFields F;
	F.flags = second ? paired_flags(false, rc2, rc1, !m1) : paired_flags(true, rc1, rc2, !m2);
	if (proper) F.flags |= 2u;
	F.mate_mapped = second ? m1 : m2;
	F.mate_seq_index = second ? r1.seq_index : r2.seq_index;
	F.mate_coord = second ? r1.coord : r2.coord;
	F.tlen = second ? tlen2 : tlen1;
	return F;
}

// The merged CIGAR runs of a path, seen from both ends: N of them, the first three (fo / fl) and the last three (lo / ll, [2] = the
// last), and the characters they print as.
struct CigarEnds {
	uint32_t N, chars;
	char fo[3], lo[3];
	uint32_t fl[3], ll[3];
};
__device__ __forceinline__ uint32_t dev_digits(uint32_t v) {
	return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u
	     : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ void cigar_ends(const urmapx_path_op *ops, uint32_t nops, CigarEnds &E) {
	E.N = 0; E.chars = 0;
	for (int t = 0; t < 3; ++t) { E.fo[t] = 0; E.lo[t] = 0; E.fl[t] = 0; E.ll[t] = 0; }
	char cur = 0;
	uint32_t curlen = 0;
	bool have = false;
	auto close_run = [&]() {
		if (E.N < 3) { E.fo[E.N] = cur; E.fl[E.N] = curlen; }
		E.lo[0] = E.lo[1]; E.ll[0] = E.ll[1]; E.lo[1] = E.lo[2]; E.ll[1] = E.ll[2]; E.lo[2] = cur; E.ll[2] = curlen;
		E.chars += dev_digits(curlen) + 1u;
		++E.N;
	};
	for (uint32_t i = 0; i < nops; ++i) {
		const uint32_t code = ops[i] & 3u, len = ops[i] >> 2;
		const char c = code == 0 ? 'M' : code == 1 ? 'I' : 'D';
		if (have && cur == c) curlen += len;
		else {
			if (have) close_run();
			cur = c; curlen = len; have = true;
		}
	}
	if (have) close_run();
}

// The op walk of both record writers: emit(len, op) for every run the CIGAR has once CIGAROpsFixDanglingMs (cigar.cpp:141-199) has
// been through it, in order.  E: cigar_ends of the same path (how many merged runs, the first three, the last three: head rule XOR
// tail rule, as in sam.cpp).  The SAM head builder prints the runs, the BAM encoder packs them.
template <class Emit>
__device__ __forceinline__ void walk_cigar_runs(const urmapx_path_op *ops, uint32_t nops, const CigarEnds &E, Emit emit) {
	const bool head_rule = E.N >= 3 && E.fo[0] == 'M' && E.fl[0] <= 2 && E.fl[1] > 4 && E.fo[2] == 'M';
	const bool tail_rule = !head_rule && E.N >= 3 && E.lo[2] == 'M' && E.ll[2] <= 2 && E.ll[1] > 4 && E.lo[0] == 'M';
	uint32_t k = 0;  // index of the merged run being closed
	char cur = 0;
	uint32_t curlen = 0;
	bool have = false;
	auto close_run = [&]() {
		uint32_t len = curlen;
		bool skip = false;
		if (head_rule) { if (k == 0) skip = true; else if (k == 2) len += E.fl[0]; }
		if (tail_rule) { if (k == E.N - 1) skip = true; else if (k == E.N - 3) len += E.ll[2]; }
		if (!skip) emit(len, cur);
		++k;
	};
	for (uint32_t i = 0; i < nops; ++i) {
		const uint32_t code = ops[i] & 3u, len = ops[i] >> 2;
		const char c = code == 0 ? 'M' : code == 1 ? 'I' : 'D';  // path D (query only) is CIGAR I and vice versa (cigar.cpp:22-25)
		if (have && cur == c) curlen += len;
		else {
			if (have) close_run();
			cur = c; curlen = len; have = true;
		}
	}
	close_run();
}

// what a record has besides its result: where its lines are, QNAME length ("/1" "/2" dropped, cut at the first blank:
// setsam.cpp:36-46), SetSAM's mate arguments
struct RecView {
	const uint8_t *raw;
	uint32_t s1, e1, e3, QL;
	MateFields F;
};
__device__ __forceinline__ RecView record_view(const SamArgs &A, uint32_t i, const urmapx_result &r) {
	RecView V;
	const uint32_t side = A.paired ? (i & 1u) : 0u, rec = A.paired ? (i >> 1) : i;
	V.raw = A.raw[side];
	const uint32_t *ends = A.ends[side];
	V.s1 = line_start(ends, 4 * rec); V.e1 = ends[4 * rec];
	const uint32_t e2 = ends[4 * rec + 1];
	V.e3 = ends[4 * rec + 2];
	V.QL = e2 - (V.e1 + 1u);
	V.F.flags = 0; V.F.mate_mapped = false; V.F.mate_seq_index = 0; V.F.mate_coord = 0xFFFFFFFFu; V.F.tlen = 0;
	if (A.paired) {
		const urmapx_result rm = A.results[i ^ 1u];
		const uint32_t *oe = A.ends[side ^ 1u];
		const uint32_t QLm = oe[4 * rec + 1] - (oe[4 * rec] + 1u);
		V.F = side ? pair_fields(rm, r, QLm, V.QL, true) : pair_fields(r, rm, V.QL, QLm, false);
	}
	return V;
}

// 4-bit code of a SEQ letter: "=ACMGRSVTWYHKDBN", either case; every other byte is N (htslib's seq_nt16_table)
__device__ __forceinline__ uint32_t nibble_of(uint32_t c) {
	if (c - (uint32_t)'a' < 26u) c -= 32u;
	const char t[] = "=ACMGRSVTWYHKDBN";
	uint32_t v = 15u;
#pragma unroll
	for (uint32_t k = 0; k < 16u; ++k)
		if (c == (uint32_t)t[k]) v = k;
	return v;
}

__device__ __forceinline__ uint32_t bcast(uint32_t v, int t) { return (uint32_t)__builtin_amdgcn_readlane((int)v, t); }

}  // namespace
#endif
