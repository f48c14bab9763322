// bam_sort.h -- what the two coordinate sorts of BAM records share (urmapx_bam_sort in bam_sort.hip, urmapx_bam_sort_host in
// bam_sort_host.cpp; include/urmapx.h "Sorted BAM output"): the key of a record, the bin of a region, the arrays an index is made
// of and the function that writes them down as a .bai file.  Not installed.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/urmapx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BAMSORT_HD __host__ __device__ __forceinline__
#else
#define BAMSORT_HD inline
#endif

namespace urx {
namespace bamsort {

constexpr uint32_t MEMBER = 65280;      // bytes of the record stream in one BGZF member
constexpr uint32_t PSEUDO_BIN = 37450;  // SAM/BAM specification v1 section 5.2: the bin that carries a reference's extent and counts
constexpr uint32_t CORE = 36;           // block_size and the eight core words
constexpr uint32_t WINDOW_SHIFT = 14;   // the linear index has one entry per 16 384 bases
constexpr uint64_t NONE = ~(uint64_t)0;

// a record starts at any byte address
BAMSORT_HD uint32_t load_u32(const uint8_t *p) {
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The BAI scheme covers [0, INDEX_END) of a reference.  A placed record that begins at or beyond it gets no chunk and no window; one
// that begins below and ends beyond is indexed as [pos, INDEX_END): the bin of that region, the windows pos >> 14 .. 32 767.  So no
// ordinary bin exceeds NO_BIN - 1 = 37 448 and no linear index has more than 32 768 entries.  Both sorts index with these two.
constexpr uint64_t INDEX_END = (uint64_t)1 << 29;
constexpr uint32_t BIN_BITS = 16;         // bits of a bin in the second sort's key
constexpr uint32_t NO_BIN = 0xFFFFu;      // there: a record without a chunk; sorts behind every bin of its reference
BAMSORT_HD bool indexed(uint64_t pos) { return pos < INDEX_END; }
BAMSORT_HD uint64_t index_end(uint64_t end) { return end < INDEX_END ? end : INDEX_END; }

// section 5.3 with 64-bit arithmetic, for [beg, end) inside [0, INDEX_END)
BAMSORT_HD uint32_t reg2bin(uint64_t beg, uint64_t end) {
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1u << 15) - 1u) / 7u + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t)(((1u << 12) - 1u) / 7u + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t)(((1u << 9) - 1u) / 7u + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t)(((1u << 6) - 1u) / 7u + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t)(((1u << 3) - 1u) / 7u + (beg >> 26));
	return 0u;
}

// CIGAR ops that advance the reference: M D N = X
BAMSORT_HD bool consumes_ref(uint32_t op) { return op == 0u || op == 2u || op == 3u || op == 7u || op == 8u; }

// bits that hold every value of 0..maxv (at least one)
BAMSORT_HD uint32_t bits_for(uint64_t maxv) {
	uint32_t b = 1;
	while (b < 64u && (maxv >> b)) ++b;
	return b;
}

// How a run packs its sort key.  A record's order is (refID as unsigned, pos as unsigned, input order).  refID is -1 or below n_ref and
// pos is -1 or at most max_pos (scan_records refuses everything else), so -1 is renamed to the value behind the largest one: the order
// stays, and the key needs bits_for(n_ref) + bits_for(max_pos + 1) bits instead of 64.
struct KeyLayout {
	uint32_t n_ref = 0, max_pos = 0, pos_bits = 1, ref_bits = 1;
	BAMSORT_HD uint32_t bits() const { return pos_bits + ref_bits; }
	BAMSORT_HD uint64_t key(uint32_t ref_id, uint32_t pos) const {
		const uint64_t r = ref_id == 0xFFFFFFFFu ? n_ref : ref_id, p = pos == 0xFFFFFFFFu ? (uint64_t)max_pos + 1u : pos;
		return r << pos_bits | p;
	}
	BAMSORT_HD uint32_t ref_of(uint64_t key) const { return (uint32_t)(key >> pos_bits); }  // n_ref: no reference
	BAMSORT_HD uint64_t pos_of(uint64_t key) const { return key & (((uint64_t)1 << pos_bits) - 1u); }  // max_pos + 1: no position
};
inline KeyLayout key_layout(uint32_t n_ref, uint32_t max_pos) {
	KeyLayout K;
	K.n_ref = n_ref; K.max_pos = max_pos;
	K.pos_bits = bits_for((uint64_t)max_pos + 1u);
	K.ref_bits = bits_for(n_ref);
	return K;
}

// The end of a record on its reference: pos + the bases its CIGAR spans there, pos + 1 without any, 2^31 at the most.  `len` is the record's whole
// length; a CIGAR that does not lie inside it counts as empty (scan_records has refused such a record before this is called).
BAMSORT_HD uint64_t ref_end(const uint8_t *rec, uint32_t len, uint64_t pos) {
	const uint32_t w3 = load_u32(rec + 12), w4 = load_u32(rec + 16);
	const uint32_t l_name = w3 & 0xFFu, n_cigar = w4 & 0xFFFFu;
	uint64_t span = 0;
	if ((uint64_t)CORE + l_name + 4ull * n_cigar <= len) {
		const uint8_t *c = rec + CORE + l_name;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t w = load_u32(c + 4u * k);
			if (consumes_ref(w & 15u)) span += w >> 4;
		}
	}
	const uint64_t end = pos + (span ? span : 1u), top = (uint64_t)1 << 31;  // (positions are below 2^31, so no end lies beyond)
	return end < top ? end : top;
}

// ---- the index, in offsets of the uncompressed sorted record stream ----
struct Chunk {  // a maximal run of records of one bin that follow one another in the file
	uint32_t ref, bin;
	uint64_t beg, end;
};
struct RefExtent {  // the pseudo-bin: where the reference's records begin and end, how many there are
	uint64_t beg = 0, end = 0, n_mapped = 0, n_unmapped = 0;
};
struct IndexArrays {
	std::vector<Chunk> chunks;      // by (ref, bin, beg); placed records only
	std::vector<uint64_t> win_base; // n_ref + 1: reference r has windows lin[win_base[r] .. win_base[r + 1])
	std::vector<uint64_t> lin;      // smallest offset of a record that overlaps the window, NONE where there is none
	std::vector<RefExtent> refs;    // n_ref
	uint64_t n_no_coor = 0;
};

// start offset of every record (n + 1 entries), the largest pos; URMAPX_E_FORMAT for bytes that are no chain of records this sort takes:
// a block_size that does not hold its own fields or runs past the end, a refID outside -1 .. n_ref - 1, a pos below -1
// starts[n_starts]: known record starts (ascending; 0 is added); the pieces between them are walked side by side
int scan_records(const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, std::vector<uint64_t> &offs, uint32_t &max_pos);
// file offset of every member of `bgzf` (from their BSIZE fields) when `in_front` bytes precede the first; one entry more: where the
// next member -- the end-of-file one -- begins.  false: not a chain of BGZF members
bool member_table(const uint8_t *bgzf, size_t n, uint64_t in_front, std::vector<uint64_t> &coffs);
// the .bai file (section 5.2): a stream offset u becomes coffs[u / MEMBER] << 16 | u % MEMBER; empty windows take the next one's value
std::vector<uint8_t> write_bai(const IndexArrays &X, uint32_t n_ref, const std::vector<uint64_t> &coffs);
// The last step of both sorts: `bgzf` (from malloc; the result owns it from here on, also when this fails) and the index arrays
// become out->bgzf and out->bai.  URMAPX_E_NOMEM; URMAPX_E_FORMAT if the members do not hold stream_bytes.
int finish_result(urmapx_bam_sort_result *out, uint8_t *bgzf, size_t bgzf_bytes, uint64_t stream_bytes, uint64_t in_front,
                  const IndexArrays &X, uint32_t n_ref);

// ---- the device sort's memory, as the plan (urmapx_bam_sort_plan_for, bam_sort_host.cpp) and the allocations (bam_sort.hip) count it ----
constexpr uint32_t DEFAULT_SLICE = 2048;           // members of 65 280 bytes in one slice of the sorted stream
constexpr uint64_t DEFAULT_STAGE = 16u << 20;      // bytes of one staged chunk on the external road (4, 16 and 64 MiB measured)
constexpr uint64_t SORT_PER_RECORD = 48;           // off, dst, two keys: 8 bytes each; three record-number arrays and the ends: 4 bytes each
constexpr uint64_t MARKDUP_PER_RECORD = 24;        // ends and best words: 8 bytes each; what a record is and where a pair begins: 4 bytes each
constexpr uint64_t ACTION_PER_RECORD = 1;          // external road under markdup: what becomes of a record's bit 0x400
constexpr uint64_t SORT_SLACK = (uint64_t)1 << 20; // the arrays per reference, the histograms, the scans' sums, the paddings

// URMAPX_TEST_SORT_SLICE=N: slices of N members; _PARTITION=N: the external road with partitions of N slices; _STAGE=B: staged chunks of B bytes
uint32_t slice_members();
uint64_t test_partition_slices();  // 0: not set
uint64_t test_stage_bytes();       // 0: not set
// beside a slice of the stream: its members at their worst, the compressor's staging slot per member and its token arenas (bgzf_gpu.hip)
size_t slice_scratch_bytes(size_t slice_bytes);
// Device bytes of the external road: the per-record arrays, two staging buffers, one partition, one slice's members, the compressor's
// scratch.  The one sum the plan and DeviceSort (whose allocate and sorted_stream stages allocate these pieces, a partition no larger
// than the stream) both use.
uint64_t external_device_bytes(size_t n_bytes, uint64_t n_records, bool markdup, uint64_t stage_bytes, uint64_t partition_bytes);
// the plan for staged chunks of stage_bytes (the public function passes the default; the sort, a larger one where a record needs it)
int plan_with_stage(size_t n_bytes, uint64_t n_records, bool markdup, uint64_t budget, uint64_t stage_bytes, urmapx_bam_sort_plan *plan);
uint64_t default_stage_bytes(size_t n_bytes);
// A staged chunk is a run of whole records [i0, i1) of at most stage_bytes, one record at the least; with `lookahead` record i1 (the
// first of the next chunk) is staged behind it and counts.  -> i1
inline uint64_t chunk_end(const uint64_t *offs, uint64_t n, uint64_t i0, uint64_t stage_bytes, bool lookahead) {
	uint64_t i1 = i0 + 1;
	const uint64_t la = lookahead ? 1u : 0u;
	while (i1 < n && offs[i1 + 1 + la < n ? i1 + 1 + la : n] - offs[i0] <= stage_bytes) ++i1;
	return i1;
}

// ---- duplicate marking (include/urmapx.h "Duplicate marking") ----
constexpr uint32_t FLAG_BYTE = 19;     // the byte of a record that holds bit 0x400 of its flag, as its bit 0x04
constexpr uint8_t FLAG_DUP_BIT = 0x04;
constexpr uint32_t MAX_SCORE = 0x7FFFFFFFu;  // where a record's score saturates
enum : uint8_t { MD_KEEP = 0, MD_SET = 1, MD_CLEAR = 2 };  // what becomes of a record's bit 0x400
// the host version (markdup_host.cpp): action[i] for every record of `rec` in input order, and the counters.  URMAPX_E_FORMAT for an
// eligible record whose SEQ and QUAL do not lie inside it
int markdup_host(const uint8_t *rec, const std::vector<uint64_t> &offs, std::vector<uint8_t> &action, urmapx_markdup_stats *md);


}  // namespace bamsort
}  // namespace urx
