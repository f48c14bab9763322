// bam_sort_dev.h -- what the device sort (bam_sort.hip) and the duplicate marking (markdup.hip) share on the device side: the sizes of
// the sort's grids, a device array, the stable radix sort and the exclusive scan (both defined in bam_sort.hip, where their kernels
// are), and the marking's entry.  HIP translation units only.  Not installed.
#pragma once
#include <chrono>

#include "bam_sort.h"
#include "internal.h"

namespace urx {
namespace bamsort {

constexpr int NT = 256;                   // threads of a sort workgroup: four wavefronts
constexpr uint32_t TILE = 4 * NT;         // records a workgroup takes when every workgroup takes the least
constexpr uint32_t MAX_BLOCKS = 512;      // workgroups of a sort pass: beyond MAX_BLOCKS * TILE records each takes several tiles
constexpr uint32_t SCAN_NT = 1024;
constexpr uint32_t MAX_RUNS = 65536;      // threads of a large scan

extern thread_local double t_alloc_s;  // what this thread's call has spent in hipMalloc and hipFree (urmapx_bam_sort_result.alloc_s)

// device array of exactly the size asked for
template <class T>
struct Dev {
	T *p = nullptr;
	int alloc(size_t n) {
		urx::AllocTimer at(0);
		const auto t0 = std::chrono::steady_clock::now();
		const hipError_t e = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T));
		t_alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return urx::hip_rc(e); }
		return URMAPX_OK;
	}
	~Dev() {
		if (!p) return;
		urx::AllocTimer at(0);
		const auto t0 = std::chrono::steady_clock::now();
		(void)hipFree(p);
		t_alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	}
};

inline uint32_t grid_for(uint64_t n, uint32_t most = 4096) {
	const uint64_t g = (n + NT - 1) / NT;
	return (uint32_t)(g < 1 ? 1 : g > most ? most : g);
}

// out[0 .. n] = exclusive sums of in[0 .. n), the total in out[n] (out is not in); sums: MAX_RUNS + 1 entries of scratch
template <class TI, class TO>
void scan_launch(const TI *in, uint32_t n, TO *out, uint64_t *sums);
extern template void scan_launch<uint32_t, uint64_t>(const uint32_t *, uint32_t, uint64_t *, uint64_t *);
extern template void scan_launch<uint32_t, uint32_t>(const uint32_t *, uint32_t, uint32_t *, uint64_t *);

// stable sort of (key, val)[0 .. n) by the low `bits` bits of the key, between two pairs of arrays; `in` says where the result is.
// hist: 256 * MAX_BLOCKS entries of scratch.  -> the histogram-scan-scatter rounds it took
struct SortArrays {
	uint64_t *key[2];
	uint32_t *val[2];
	int in = 0;
};
uint32_t radix_sort(SortArrays &S, uint32_t n, uint32_t bits, uint32_t *hist);

// The marking (markdup.hip) in two steps.
// 1. What it reads of the records' bytes -- ends, scores, refIDs, which neighbours are pairs -- goes into its own arrays (24 bytes a
//    record: MarkdupOwn), a chunk of records at a time: records i0 .. i1 - 1 lie at rec + (off[i] - base), and unless i1 is n record i1
//    lies behind them.  In core that is one chunk of all records (base 0) just before step 2; on the external road every staged chunk of
//    the first pass, so begin() comes before that pass.
// 2. Inside the device sort once the index arrays are made and before the first record is copied into order: the groups and the
//    decisions, from the arrays alone.  Bit 0x400 of the eligible records is set or cleared in `rec` (n records at off[0 .. n], as they
//    came), or, with `action` (n bytes, MD_KEEP at first; rec unused), the decision is stored there.  The counters go to md.  key / val:
//    the sort's two key arrays (n + 2 entries each) and two of its record-number arrays (n + 1), free by then; score: n entries (the
//    sort's array of ends); hist, sums: as above.
struct MarkdupOwn {
	Dev<uint64_t> end, best;
	Dev<uint32_t> what, first;
	Dev<unsigned long long> stat;
	int begin(uint32_t n);  // the arrays and the statistics block
};
int markdup_chunk(const MarkdupOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, uint32_t n, hipStream_t stream);
struct MarkdupArrays {
	uint8_t *rec;
	const uint64_t *off;
	uint32_t n, n_ref;
	uint64_t *key[2];
	uint32_t *val[2];
	uint32_t *score, *hist;
	uint64_t *sums;
	uint8_t *action;
};
int markdup_device(const MarkdupArrays &A, const MarkdupOwn &W, urmapx_markdup_stats *md);

}  // namespace bamsort
}  // namespace urx
