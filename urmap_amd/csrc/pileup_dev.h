// pileup_dev.h -- the device side of the pileup (pileup.hip) as its two callers see it: urmapx_bam_pileup, which streams the records
// through staging buffers (staged_alone), and the device sort (bam_sort.hip, urmapx_bam_sort_with), which has them on the device anyway.
// HIP translation units only.  Not installed.
#pragma once
#include "bam_sort_dev.h"
#include "pileup.h"

namespace urx {
namespace pileup {

using bamsort::Dev;

// the arrays resident_bytes (pileup.h) counts, allocated in its order
struct PileupOwn {
	Dev<uint4> cnt;                     // a column's counters A, C, G, T; reference r owns entries base[r] .. base[r + 1] - 1
	Dev<uint64_t> base;                 // n_ref + 1
	Dev<uint64_t> seq_at;               // n_ref + 1: where reference r's bases begin in `seq`
	Dev<uint32_t> bcount;               // a count per workgroup of one segment of the site search, then their exclusive sums and the total
	Dev<Site> sites[2];                 // two slices of entries
	Dev<uint8_t> bases;                 // the uploaded bases (not with a resident store)
	Dev<unsigned long long> stat;       // records that counted
	const uint8_t *seq = nullptr;       // the bases: `bases`, or the resident store
	uint64_t columns = 0, segment = 0;
	uint32_t n_ref = 0, slice = 0, blocks = 1;  // workgroups of pileup_count_kernel at the most (URMAPX_TEST_PILEUP_BLOCKS: fewer)
	// The arrays on the current device, the counters zero.  The bases: seqs (host, lens[r] letters each; checked by check_input) are
	// uploaded, or, with seqs null, d_store is read in place, reference r's letters from d_store + store_at[r] on
	int begin(uint32_t n_ref_, const uint32_t *lens, uint64_t columns_, const uint8_t *const *seqs, const uint8_t *d_store, const uint64_t *store_at);
};
// Records i0 .. i1 - 1 lie at rec + (off[i] - base), as for keys_kernel; action (optional): the marking's decision per record (MD_*),
// which stands in for bit 0x400.  Queues pileup_count_kernel on `stream`.
int pileup_count(const PileupOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, const Rule &R,
                 hipStream_t stream);
// once every record is counted: the sites, segment by segment and slice by slice, and the text into out (text, text_bytes, sites,
// alt_alleles, records, sites_s, format_s, copy_s)
int pileup_finish(PileupOwn &W, const char *const *names, const uint32_t *lens, const Rule &R, const char *command, urmapx_pileup_result *out);

// The pileup as a by-product of the staged pass (include/urmapx.h "Pileup"); names, lens and the rule are checked.  The bases: seqs on
// the host, or, with seqs null, d_store on the current device with reference r's letters from store_at[r] on
struct PileupBeside final : bamsort::Beside {
	const uint32_t n_ref;
	const Rule R;
	const char *const *const names;
	const uint32_t *const lens;
	const uint64_t columns;
	const uint8_t *const *const seqs;
	const uint8_t *const d_store;
	const uint64_t *const store_at;
	const char *const command;
	urmapx_pileup_result *const out;
	PileupOwn W;
	PileupBeside(uint32_t n_ref_, const Rule &R_, const char *const *names_, const uint32_t *lens_, uint64_t columns_, const uint8_t *const *seqs_,
	             const uint8_t *d_store_, const uint64_t *store_at_, const char *command_, urmapx_pileup_result *out_)
	    : Beside(&out_->least_budget, &out_->alloc_s, &out_->count_s), n_ref(n_ref_), R(R_), names(names_), lens(lens_), columns(columns_), seqs(seqs_),
	      d_store(d_store_), store_at(store_at_), command(command_), out(out_) {}
	uint64_t resident_bytes() const override;
	int begin(uint32_t n) override;
	int count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) override;
	int finish() override;
	void free_result() override;
};

}  // namespace pileup
}  // namespace urx
