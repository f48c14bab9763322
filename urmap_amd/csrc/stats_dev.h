// stats_dev.h -- the device side of the alignment statistics (stats.hip) as its two callers see it: urmapx_bam_stats, which streams the
// records through staging buffers (staged_alone), and the device sort (bam_sort.hip, urmapx_bam_sort_with), which has them on the
// device anyway.  HIP translation units only.  Not installed.
#pragma once
#include "bam_sort_dev.h"
#include "stats.h"

namespace urx {
namespace stats {

using bamsort::Dev;

// the array resident_bytes (stats.h) counts
struct StatsOwn {
	Dev<unsigned long long> tab;  // table_words(n_ref) words: the layout of stats.h
	uint32_t n_ref = 0, blocks = 1;  // workgroups of a launch at the most: one per compute unit (URMAPX_TEST_STATS_BLOCKS: fewer)
	int begin(uint32_t n_ref_);   // the tables on the current device, zero
};
// Records i0 .. i1 - 1 lie at rec + (off[i] - base), as for keys_kernel; action (optional): the marking's decision per record (MD_*),
// which stands in for bit 0x400.  Queues stats_count_kernel on `stream`, once per LAUNCH_RECORDS records.
int stats_count(const StatsOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream);
// once every record is counted: the tables back and the text into out (text, text_bytes, the totals, format_s)
int stats_finish(StatsOwn &W, const char *const *names, const uint32_t *lens, const char *command, urmapx_stats_result *out);

// the statistics as a by-product of the staged pass (include/urmapx.h "Stats"); names and lens are checked
struct StatsBeside final : bamsort::Beside {
	const uint32_t n_ref;
	const char *const *const names;
	const uint32_t *const lens;
	const char *const command;
	urmapx_stats_result *const out;
	StatsOwn W;
	StatsBeside(uint32_t n_ref_, const char *const *names_, const uint32_t *lens_, const char *command_, urmapx_stats_result *out_)
	    : Beside(&out_->least_budget, &out_->alloc_s, &out_->count_s), n_ref(n_ref_), names(names_), lens(lens_), command(command_), out(out_) {}
	uint64_t resident_bytes() const override;
	int begin(uint32_t n) override;
	int count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) override;
	int finish() override;
	void free_result() override;
};

}  // namespace stats
}  // namespace urx
