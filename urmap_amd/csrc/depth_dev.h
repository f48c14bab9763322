// depth_dev.h -- the device side of the depth computation (depth.hip) as its two callers see it: urmapx_bam_depth, which streams the
// records through staging buffers (staged_alone), and the device sort (bam_sort.hip, urmapx_bam_sort_with), which has them on the
// device anyway.  HIP translation units only.  Not installed.
#pragma once
#include "bam_sort_dev.h"
#include "depth.h"

namespace urx {
namespace depth {

using bamsort::Dev;

// the arrays resident_bytes (depth.h) counts, allocated in its order
struct DepthOwn {
	Dev<uint32_t> diff;                 // the counters: differences until the scan, depths after it
	Dev<uint64_t> base;                 // n_ref + 1: reference r owns counters base[r] .. base[r + 1] - 1, the last one for ends beyond it
	Dev<uint8_t> names;                 // n_ref slots of NAME_SLOT bytes
	Dev<unsigned long long> stat;       // per reference: reads, covered, bases, mapq_sum (urmapx_depth_summary)
	Dev<uint64_t> list;                 // run starts of a segment: one carried over in front, the next start or the end behind
	Dev<uint32_t> bcount, ssum;
	Dev<uint8_t> text[2];
	Dev<uint32_t> llen[2];
	Dev<uint64_t> loff[2];
	uint64_t entries = 0;
	uint32_t n_ref = 0, slice_runs = 0;
	// the arrays, the references' table and names on the device, the counters zero.  names and lens: checked by check_refs
	int begin(uint32_t n_ref_, const char *const *names_, const uint32_t *lens, uint64_t entries_);
};
// Records i0 .. i1 - 1 lie at rec + (off[i] - base), as for keys_kernel; action (optional): the marking's decision per record (MD_*),
// which stands in for bit 0x400.  Queues depth_count_kernel on `stream`.
int depth_count(const DepthOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, uint32_t min_mapq,
                hipStream_t stream);
// once every record is counted: the scan, the runs, the text and the summaries into out (text, text_bytes, runs, refs, n_ref,
// text_slices and the times but count_s and alloc_s)
int depth_finish(DepthOwn &W, urmapx_depth_result *out);

// the depth as a by-product of the staged pass (include/urmapx.h "Depth"); names and lens are checked (check_refs: entries)
struct DepthBeside final : bamsort::Beside {
	const uint32_t n_ref, min_mapq;
	const char *const *const names;
	const uint32_t *const lens;
	const uint64_t entries;
	urmapx_depth_result *const out;
	DepthOwn W;
	DepthBeside(uint32_t n_ref_, const char *const *names_, const uint32_t *lens_, uint64_t entries_, uint32_t min_mapq_, urmapx_depth_result *out_)
	    : Beside(&out_->least_budget, &out_->alloc_s, &out_->count_s), n_ref(n_ref_), min_mapq(min_mapq_), names(names_), lens(lens_), entries(entries_), out(out_) {}
	uint64_t resident_bytes() const override;
	int begin(uint32_t n) override;
	int count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) override;
	int finish() override;
	void free_result() override;
};

}  // namespace depth
}  // namespace urx
