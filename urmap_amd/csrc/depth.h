// depth.h -- what the two depth computations share (urmapx_bam_depth in depth.hip, urmapx_bam_depth_host in depth_host.cpp; the rule
// is in include/urmapx.h "Depth"): the sizes of the device version's grids, slices and lines, and the one sum of device bytes that
// both the public functions and the allocations follow.  Not installed.
#pragma once
#include "bam_sort.h"

namespace urx {
namespace depth {

constexpr uint32_t NT = 256;                       // threads of a depth workgroup: four wavefronts
constexpr uint32_t COUNT_BLOCKS = 1024;            // workgroups of depth_count_kernel at the most: beyond COUNT_BLOCKS * NT records a thread takes several
constexpr uint32_t LANE_OPS = 8;                   // CIGAR ops a lane walks alone; a longer CIGAR is shared by its wavefront, 64 ops at a time
constexpr uint32_t SCAN_ITEMS = 8;                 // counters a thread scans at a time
constexpr uint32_t SCAN_TILE = NT * SCAN_ITEMS;    // counters a workgroup scans at a time
constexpr uint32_t SCAN_BLOCKS = 1024;             // workgroups of the scan: beyond SCAN_BLOCKS * SCAN_TILE counters each takes several tiles
constexpr uint32_t RUN_TILE = SCAN_TILE;           // counters whose run starts a workgroup finds
constexpr uint32_t RUN_BLOCKS = 1024;              // workgroups of one segment of the run search
constexpr uint64_t SEGMENT = (uint64_t)RUN_TILE * RUN_BLOCKS;  // counters whose run starts lie on the device at a time
constexpr uint32_t TEXT_RUNS = 65536;              // lines of one slice of the text
constexpr uint32_t MAX_NAME = 255;                 // bytes of a reference name
constexpr uint32_t NAME_SLOT = MAX_NAME + 1;       // a name on the device: its length, then its bytes
constexpr uint32_t LINE_MOST = MAX_NAME + 4 + 3 * 10;  // name, three tabs and the newline, three numbers below 2^32
constexpr uint64_t DEPTH_SLACK = (uint64_t)1 << 20;    // the paddings of the arrays and the words that carry a total or a run across

// URMAPX_TEST_DEPTH_SLICE=N: text slices of N lines
uint32_t text_runs();

// the counters: reference r owns l_ref + 1 of them
inline uint64_t entries_of(uint64_t total_columns, uint32_t n_ref) { return total_columns + n_ref; }

// Device bytes of the depth arrays, in the order DepthOwn::begin (depth.hip) allocates them: the counters; where every reference's
// begin; the names; the four sums per reference; the run starts of one segment (and the one carried over, and the end); a count per
// workgroup of the run search and a sum per workgroup of the scan; two slices of text with their line lengths and line starts.
inline uint64_t resident_bytes(uint64_t entries, uint32_t n_ref, uint32_t slice_runs) {
	const uint64_t seg = entries < SEGMENT ? entries : SEGMENT;
	return 4u * entries + 8u * ((uint64_t)n_ref + 1u) + (uint64_t)NAME_SLOT * n_ref + 32u * (uint64_t)n_ref + 8u * (seg + 2u) +
	       4u * (uint64_t)(RUN_BLOCKS + 1u) + 4u * (uint64_t)(SCAN_BLOCKS + 1u) +
	       2u * ((uint64_t)slice_runs * LINE_MOST + 4u * (uint64_t)slice_runs + 8u * ((uint64_t)slice_runs + 1u)) + DEPTH_SLACK;
}
// urmapx_bam_depth adds the record starts and two staging buffers
inline uint64_t standalone_bytes(uint64_t entries, uint32_t n_ref, uint32_t slice_runs, uint64_t n_records, uint64_t stage_bytes) {
	return resident_bytes(entries, n_ref, slice_runs) + 8u * (n_records + 1u) + 2u * (stage_bytes + 16u);
}

// names of 1 .. MAX_NAME bytes, lengths given (URMAPX_E_ARG); -> the counters' count
int check_refs(uint32_t n_ref, const char *const *names, const uint32_t *lens, uint64_t *entries);
// scan_records, with 2^31 records or more told apart from a broken chain: URMAPX_E_ARG
int scan_for_depth(const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, std::vector<uint64_t> &offs);
// the host version on scanned records; action (optional): the marking's decisions, as markdup_host makes them
int depth_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
               uint32_t min_mapq, urmapx_depth_result *out);

}  // namespace depth
}  // namespace urx
