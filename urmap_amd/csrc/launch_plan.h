// launch_plan.h -- what the single-end launcher decides before it enqueues anything: the read-length class, the search kernel's
// instance and phase 6's rounds.  Host only and free of HIP: tests/tools/launch_plan_main.cpp compiles it with g++ and prints the table.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

namespace urx {

// The read-length class of a batch: 0..5 = reads of up to 128, 192, 256, 320, 512, 1024 bases; -1 beyond.  One numbering for the
// per-class caches of the context (blocks[], dp_blocks[], fin_blocks[], pe_blocks[]) and for the kernels' template argument.
static constexpr int READ_CLASSES = 6;
inline int read_class(uint32_t max_read_len) {
	return max_read_len <= 128 ? 0 : max_read_len <= 192 ? 1 : max_read_len <= 256 ? 2 : max_read_len <= 320 ? 3 : max_read_len <= 512 ? 4 : max_read_len <= 1024 ? 5 : -1;
}
// NCH, the 64-base chunks of the class's longest read (0: no class).  2: two mask words, 8 window loads; 4: smaller per-read state than
// the 320-base class, one more wave per SIMD; 8 and 16: 1 wave per SIMD, eight mask words and 32 window loads per lane and up
inline int nch_for(uint32_t max_read_len) {
	constexpr int nch[READ_CLASSES] = {2, 3, 4, 5, 8, 16};
	const int c = read_class(max_read_len);
	return c < 0 ? 0 : nch[c];
}

// The runtime class as a compile-time constant: f(std::integral_constant<int, N>) for the N of the list that equals nch.  A value outside
// the list takes the last one (what the final else of the launchers' ladders did).
template <int N, int... Rest, class F>
inline auto dispatch_nch(int nch, F &&f) {
	if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, N>{});
	else {
		if (nch == N) return f(std::integral_constant<int, N>{});
		return dispatch_nch<Rest...>(nch, f);
	}
}

// The jobs of a read are run in rounds of growing size, [0,2) [2,16) [16,inf) by index: after each round the ordered
// replay consumes that round's jobs and the penalty cap it arrives at gates the next round's DPs -- most of a repeat
// read's HSPs fail AlignHSP's first test once the first few alignments have tightened the cap.
// Round 5: the boundaries are chosen per call (SearchWork::dp_bounds): [0,2) [2,16) [16,inf) for reads of up to 192 bases, [0,2) [2,8)
// [8,32) [32,inf) beyond (250-base reads with 5 % errors bring 13 HSPs each to phase 6: the fourth round's tighter gate is worth more
// than its two launches cost -- measured in round 4).  DP_ROUNDS = the most rounds a call may have.
static constexpr int DP_ROUNDS = 4;
struct DpBounds {
	int rounds;                    // rounds in use, 1 .. DP_ROUNDS
	uint32_t lo[DP_ROUNDS + 1];    // round rd = jobs with lo[rd] <= k < lo[rd + 1]; lo[rounds] = 0xFFFFFFFF, unused rounds are empty
};
inline DpBounds dp_bounds_default(bool long_reads) {
	DpBounds b;
	if (long_reads) { b.rounds = 4; b.lo[0] = 0; b.lo[1] = 2; b.lo[2] = 8; b.lo[3] = 32; b.lo[4] = 0xFFFFFFFFu; }
	else { b.rounds = 3; b.lo[0] = 0; b.lo[1] = 2; b.lo[2] = 16; b.lo[3] = 0xFFFFFFFFu; b.lo[4] = 0xFFFFFFFFu; }
	return b;
}
// URMAPX_DP_BOUNDS="0,2,8,32" (measurement): up to DP_ROUNDS rising lower bounds, the first of them 0; anything else (and e == nullptr)
// leaves `fallback`
inline DpBounds parse_dp_bounds(const char *e, const DpBounds &fallback) {
	DpBounds b;
	b.rounds = 0;
	for (const char *c = e; c && *c && b.rounds < DP_ROUNDS;) {
		char *end;
		const unsigned long v = strtoul(c, &end, 10);
		if (end == c) break;
		b.lo[b.rounds++] = (uint32_t)v;
		c = *end == ',' ? end + 1 : end;
	}
	bool ok = b.rounds >= 1 && b.lo[0] == 0;
	for (int i = 1; i < b.rounds; ++i) ok = ok && b.lo[i] > b.lo[i - 1];
	if (!ok) return fallback;
	for (int i = b.rounds; i <= DP_ROUNDS; ++i) b.lo[i] = 0xFFFFFFFFu;
	return b;
}

// The first pass of launch_search_se, one of:
enum class FirstPass {
	ParkedPhase3,  // three launches: the search without banded DP (PART 1), phase 3's flank DPs, the search over the reads parked there (PART 2)
	Slot16,        // slots, row lengths and second positions in one gather (DevIndex::slot16)
	Slot16K2,      // the same with two chunks of k-mer starts and the row store in LDS: 150-base reads
	Diagnostic,    // per-phase cycle counters (URMAPX_PHASE_STATS / URMAPX_DEBUG_STOP), phase 6 inline: the 150 / 250 bp classes only
	Rows,          // the chain rows are looked up in the layout built with the index (DevIndex::rowinfo)
	Hops,          // chains walked hop by hop
};
struct SearchPlanIn {
	int nch;                     // nch_for(max_read_len)
	bool rowinfo, slot16;        // which layouts of the index are resident
	bool stats, dp0, dp3;        // SearchWork::stats is set; SearchWork::dp[0] / dp3 have job arrays
	int dp_blocks;
	uint32_t max_read_len, W;
	bool no_k2;                  // URMAPX_NO_K2 (A/B, tests)
};
struct SearchPlan {
	FirstPass first;
	bool phase6_launches;  // phase 6 of the first pass's reads runs as launches of its own (the second pass's: whenever dp[1] has a job array)
};
inline SearchPlan plan_search_se(const SearchPlanIn &in) {
	const bool diag = in.stats && (in.nch == 3 || in.nch == 4);
	// round 6: every read of the batch has at most 128 k-mer starts (150 bases at W = 24): the instance that keeps two chunks of them
	const bool k2 = !in.no_k2 && in.max_read_len >= in.W && in.max_read_len - (in.W - 1) <= 128u;
	SearchPlan p;
	p.phase6_launches = in.dp0 && !diag;
	// phase 3 parked: reads of up to 320 bases on an index with the row layout, phase 6 as launches of its own (the default)
	if (!in.stats && in.dp3 && in.dp0 && in.dp_blocks > 0 && in.rowinfo && in.nch <= 5) p.first = FirstPass::ParkedPhase3;
	else if (!in.stats && in.slot16) p.first = in.nch == 3 && k2 ? FirstPass::Slot16K2 : FirstPass::Slot16;
	else if (diag) p.first = FirstPass::Diagnostic;
	else p.first = in.rowinfo ? FirstPass::Rows : FirstPass::Hops;
	return p;
}

// search_se_kernel's template arguments: <NCH, OVF, DBG, ROWS, PART, KCH>
struct SearchInstance { int nch; bool ovf, dbg; int rows, part, kch; };
// the instance a first-pass variant stands for (ParkedPhase3: its first launch; its second is the same with part = 2)
constexpr SearchInstance first_pass_instance(FirstPass v, int nch) {
	return v == FirstPass::ParkedPhase3 ? SearchInstance{nch, false, false, 1, 1, nch}
	       : v == FirstPass::Slot16     ? SearchInstance{nch, false, false, 2, 0, nch}
	       : v == FirstPass::Slot16K2   ? SearchInstance{nch, false, false, 2, 0, 2}
	       : v == FirstPass::Diagnostic ? SearchInstance{nch, false, true, 0, 0, nch}
	       : v == FirstPass::Rows       ? SearchInstance{nch, false, false, 1, 0, nch}
	                                    : SearchInstance{nch, false, false, 0, 0, nch};
}
// the second pass over the reads whose lists outgrew the first's: hop by hop, lists continued in global scratch
constexpr SearchInstance second_pass_instance(int nch) { return SearchInstance{nch, true, false, 0, 0, nch}; }

}  // namespace urx
