// pileup.h -- what the two pileups share (urmapx_bam_pileup in pileup.hip, urmapx_bam_pileup_host in pileup_host.cpp; the rule is in
// include/urmapx.h "Pileup"): the site entry both hand to the one formatter, the sizes of the device version's grids, segments and
// slices, and the one sum of device bytes that both the public functions and the allocations follow.  Not installed.
#pragma once
#include <string>

#include "bam_sort.h"

namespace urx {
namespace pileup {

// A site as both versions hand it to the formatter: the column counted over all references (reference r owns columns base[r] ..
// base[r] + l_ref - 1) with the reference base's number (A C G T: 0 .. 3) in its two top bits, and the four counters
struct Site {
	uint64_t column;
	uint32_t cnt[4];
};
static_assert(sizeof(Site) == 24, "the entries the device writes");
constexpr uint32_t REF_SHIFT = 62;
constexpr uint64_t COLUMN_MASK = ((uint64_t)1 << REF_SHIFT) - 1u;

// the options with the defaults in place
struct Rule {
	uint32_t min_mapq = 0, min_baseq = 13, min_alt = 3, min_pct = 10;
};
// URMAPX_E_ARG for values outside the rule's ranges; opts null: the defaults
int rule_of(const urmapx_pileup_opts *opts, Rule *R);

// the number of a 4-bit base code (1 2 4 8 -> 0 1 2 3), 4 for every other; of a reference letter, case folded
BAMSORT_HD uint32_t base_of_code(uint32_t code) { return code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : 4u; }
BAMSORT_HD uint32_t base_of_letter(uint32_t ch) {
	const uint32_t c = ch | 0x20u;
	return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : 4u;
}
// rule 3 on one column: bit b set: base b is an alternative allele (ref: 0 .. 3)
BAMSORT_HD uint32_t alt_mask(const uint32_t (&cnt)[4], uint32_t ref, uint32_t min_alt, uint32_t min_pct) {
	const uint64_t dp = (uint64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3];
	uint32_t m = 0;
	for (uint32_t b = 0; b < 4u; ++b)
		if (b != ref && cnt[b] >= min_alt && (uint64_t)cnt[b] * 100u >= (uint64_t)min_pct * dp) m |= 1u << b;
	return m;
}

// ---- the device version (pileup.hip) ----
constexpr uint32_t NT = 256;                       // threads of a workgroup: four wavefronts, a record each at a time
constexpr uint32_t WAVES = NT / 64;
constexpr uint32_t SITE_BLOCKS = 16384;            // workgroups of one segment of the site search, a column a thread
constexpr uint64_t SEGMENT = (uint64_t)NT * SITE_BLOCKS;  // columns whose sites are counted at a time
constexpr uint32_t SLICE_SITES = 1u << 18;         // site entries of one slice on their way to the host
constexpr uint64_t PILEUP_SLACK = (uint64_t)1 << 16;   // the paddings of the arrays and the counter of records

// URMAPX_TEST_PILEUP_BLOCKS=N: at most N workgroups of pileup_count_kernel (0: not set); _SEGMENT=N: segments of N columns (rounded up
// to whole workgroups); _SLICE=N: slices of N entries
uint32_t test_blocks();
uint64_t segment_columns();
uint32_t slice_sites();

// Device bytes of the pileup's arrays, in the order PileupOwn::begin (pileup.hip) allocates them: the counters; where every
// reference's begin and where its bases lie; a count per workgroup of the site search; two slices of entries; the uploaded bases
inline uint64_t resident_bytes(uint64_t columns, uint32_t n_ref, uint64_t segment, uint32_t slice, bool seq_resident) {
	const uint64_t blocks = ((columns < segment ? columns : segment) + NT - 1) / NT;
	return 16u * columns + 16u * ((uint64_t)n_ref + 1u) + 4u * (blocks + 1u) + 2u * sizeof(Site) * (uint64_t)slice + (seq_resident ? 0u : columns) + PILEUP_SLACK;
}
// urmapx_bam_pileup adds the record starts and two staging buffers
inline uint64_t standalone_bytes(uint64_t columns, uint32_t n_ref, uint64_t segment, uint32_t slice, uint64_t n_records, uint64_t stage_bytes) {
	return resident_bytes(columns, n_ref, segment, slice, false) + 8u * (n_records + 1u) + 2u * (stage_bytes + 16u);
}

// names as for the depth, a sequence for every reference with a length; -> the columns' count
int check_input(uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint8_t *const *seqs, uint64_t *columns);
// the index's sequences on the host, one after the other, where its count and lengths are n_ref and lens (URMAPX_E_ARG); ptrs[r]: into store
int index_sequences(const urmapx_index *I, uint32_t n_ref, const uint32_t *lens, std::vector<uint8_t> &store, std::vector<const uint8_t *> &ptrs);
// the text from the sites in ascending column order (both versions end here); sets text, text_bytes, sites, alt_alleles
int format_sites(const Site *sites, size_t n_sites, uint32_t n_ref, const char *const *names, const uint32_t *lens, const Rule &R, const char *command,
                 urmapx_pileup_result *out);
// the host version on scanned records; action (optional): the marking's decisions
int pileup_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                const uint8_t *const *seqs, const Rule &R, const char *command, urmapx_pileup_result *out);

}  // namespace pileup
}  // namespace urx
