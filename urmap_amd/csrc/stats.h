// stats.h -- what the two alignment-statistics computations share (urmapx_bam_stats in stats.hip, urmapx_bam_stats_host in
// stats_host.cpp; the rule is in include/urmapx.h "Stats"): the caps of the rule, the one layout of the 64-bit tables that the device
// kernel, the host loop and the formatter (stats_host.cpp) all use, the sizes of the kernel's LDS copies, and the one sum of device
// bytes that both the public function and the allocations follow.  Not installed.
#pragma once
#include <string>

#include "bam_sort.h"

namespace urx {
namespace stats {

// ---- the rule's caps: a value beyond one falls into the last bin ----
constexpr uint32_t CYCLES = 1024;   // cycles with a row of their own; the later ones share one more
constexpr uint32_t QUALS = 94;      // quality values 0 .. 93; a QUAL byte above counts as 93
constexpr uint32_t IS_MAX = 8000;   // insert sizes
constexpr uint32_t RL_MAX = 65535;  // read lengths
constexpr uint32_t ID_MAX = 256;    // indel lengths
constexpr uint32_t BASES = 6;       // A C G T N other

// ---- the SN counters as the tables hold them (the text derives the remaining lines) ----
enum : uint32_t {
	SN_RECORDS, SN_SECONDARY, SN_SUPPLEMENTARY, SN_READS, SN_PAIRED, SN_FIRST, SN_LAST, SN_MAPPED, SN_UNMAPPED, SN_PROPER, SN_MAPPED_PAIRED,
	SN_SINGLETONS, SN_MATE_OTHER, SN_REVERSE, SN_DUP, SN_QCFAIL, SN_MQ0, SN_NOQUAL, SN_TOTAL_LEN, SN_BASES_MAPPED, SN_BASES_CIGAR, SN_SOFT,
	SN_BASES_INS, SN_BASES_DEL, SN_INS, SN_DEL, SN_BASES_DUP, SN_WITH_NM, SN_MISMATCHES, SN_NM_BASES, SN_QUAL_SUM, SN_QUAL_BASES,
	SN_MAX_LEN,  // the only one that is a maximum, not a sum
	SN_USED
};
constexpr uint32_t SN_N = 64;  // a lane of a wavefront each (stats.hip)

// ---- the tables: one array of 64-bit words ----
constexpr uint64_t T_SN = 0;
constexpr uint64_t T_MQ = T_SN + SN_N;                                   // [256]
constexpr uint64_t T_GC = T_MQ + 256;                                    // [101], padded to 104
constexpr uint64_t T_ID = T_GC + 104;                                    // [ID_MAX + 1][2]: insertions, deletions
constexpr uint64_t T_IS = T_ID + 2u * (ID_MAX + 1);                      // [IS_MAX + 1][3]: inward, outward, other
constexpr uint64_t T_RL = T_IS + 3u * (IS_MAX + 1);                      // [RL_MAX + 1][2]: first, last fragments
constexpr uint64_t T_BC = T_RL + 2u * ((uint64_t)RL_MAX + 1);            // [CYCLES + 1][BASES]
constexpr uint64_t T_Q = T_BC + (uint64_t)BASES * (CYCLES + 1);          // [2][CYCLES + 1][QUALS]: first, last fragments
constexpr uint64_t T_RF = T_Q + 2ull * QUALS * (CYCLES + 1);             // [n_ref + 1][3]: mapped, unmapped, duplicated; the last row: refID -1
inline uint64_t table_words(uint32_t n_ref) { return T_RF + 3u * ((uint64_t)n_ref + 1u); }

// ---- the device version (stats.hip) ----
constexpr uint32_t NT = 1024;             // threads of a workgroup: sixteen wavefronts, a record each at a time
constexpr uint32_t LANE_OPS = 8;          // the first ops of a CIGAR, whose ID bins count in LDS; those of the later ones go to the tables directly
constexpr uint32_t LAUNCH_RECORDS = 1u << 28;  // records of one launch at the most: a 32-bit LDS bin takes at most LANE_OPS a record
// the low ends that a workgroup counts in LDS, 32 bits a bin, and adds to the tables once; what lies beyond goes to the tables directly
constexpr uint32_t L_CYCLES = 160;        // cycles of BC and of both quality tables
constexpr uint32_t L_QROW = QUALS + 1;    // words of a quality row in LDS: odd, so equal qualities of 64 cycles fall on different banks
constexpr uint32_t L_IS = 1024, L_RL = 512, L_ID = 64, L_RF = 1024;
constexpr uint32_t LDS_WORDS = 2u * L_CYCLES * L_QROW + L_CYCLES * BASES + 256u + 104u + 3u * L_IS + 2u * L_RL + 2u * L_ID + 3u * L_RF;
constexpr uint32_t LDS_BYTES = 4u * LDS_WORDS + 8u * SN_N;
static_assert(LDS_BYTES <= 160u * 1024u, "the LDS of one compute unit");
constexpr uint64_t STATS_SLACK = 4096;    // the padding of the array

// URMAPX_TEST_STATS_BLOCKS=N: at most N workgroups (0: not set)
uint32_t test_blocks();

// Device bytes of the statistics: the tables.  The one sum urmapx_bam_stats_resident_bytes, the planned sort and StatsOwn::begin follow
inline uint64_t resident_bytes(uint32_t n_ref) { return 8u * table_words(n_ref) + STATS_SLACK; }
// urmapx_bam_stats adds the record starts and two staging buffers
inline uint64_t standalone_bytes(uint32_t n_ref, uint64_t n_records, uint64_t stage_bytes) {
	return resident_bytes(n_ref) + 8u * (n_records + 1u) + 2u * (stage_bytes + 16u);
}

// the host loop: records offs[i] .. of `rec` into `tab` (table_words(n_ref) words, added to); action (optional): the marking's decisions
void count_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, uint64_t *tab);
// the text from the tables, and the totals of `out` the log line needs (both versions end here).  command: NULL counts as ""
int format_tables(const uint64_t *tab, uint32_t n_ref, const char *const *names, const uint32_t *lens, const char *command, urmapx_stats_result *out);
// the host version on scanned records
int stats_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
               const char *command, urmapx_stats_result *out);

}  // namespace stats
}  // namespace urx
