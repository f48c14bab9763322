// bam_sort_dev.h -- what the device sort (bam_sort.hip), the duplicate marking (markdup.hip) and what is taken beside the sort (depth.hip,
// stats.hip, pileup.hip) share on the device side: the sizes of the sort's grids, a device array, the stable radix sort and the
// exclusive scan (both defined in bam_sort.hip, where their kernels are), the marking's entry, and the staged pass: the two streams,
// the chunks, the pass over them, what a by-product of the pass provides (Beside) and the pass on its own.  HIP translation units only.
// Not installed.
#pragma once
#include <algorithm>
#include <chrono>
#include <vector>

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

// page-locked memory of the host
struct Pinned {
	uint8_t *p = nullptr;
	int alloc(size_t n) {
		const hipError_t e = hipHostMalloc((void **)&p, n ? n : 1, hipHostMallocDefault);
		if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return urx::hip_rc(e); }
		return URMAPX_OK;
	}
	~Pinned() {
		if (p) (void)hipHostFree(p);
	}
};

// two non-blocking streams.  Of a staged pass: a staging buffer's copy and the kernels that read it go to the buffer's own stream, so
// the kernels of one chunk run while the next chunk is copied
struct TwoStreams {
	hipStream_t s[2] = {nullptr, nullptr};
	int create() {
		for (int b = 0; b < 2; ++b) HIP_TRY(hipStreamCreateWithFlags(&s[b], hipStreamNonBlocking));
		return URMAPX_OK;
	}
	int wait() {
		for (int b = 0; b < 2; ++b)
			if (s[b]) HIP_TRY(hipStreamSynchronize(s[b]));
		return URMAPX_OK;
	}
	~TwoStreams() {
		for (int b = 0; b < 2; ++b)
			if (s[b]) (void)hipStreamDestroy(s[b]);
	}
};

// The staged chunks of records 0 .. n - 1 (starts offs[0 .. n]) for staging buffers of `stage` bytes: chunk c is records cut[c] ..
// cut[c + 1] - 1, runs of whole records, one at the least.  -> the bytes of the largest chunk, under lookahead with the next chunk's
// first record behind it: a record longer than `stage`, or its successor, makes that more than `stage`
inline uint64_t cut_chunks(const uint64_t *offs, uint32_t n, uint64_t stage, bool lookahead, std::vector<uint32_t> &cut) {
	uint64_t need = 0;
	for (uint64_t i0 = 0; i0 < n;) {
		const uint64_t i1 = chunk_end(offs, n, i0, stage, lookahead), seen = lookahead && i1 < n ? i1 + 1 : i1;
		cut.push_back((uint32_t)i0);
		need = std::max(need, offs[seen] - offs[i0]);
		i0 = i1;
	}
	cut.push_back(n);
	return need;
}

// One pass over the records at `rec` (the caller's pageable memory) in the chunks of `cut`: chunk c goes to staging buffer c & 1
// (stage_bytes each) on that buffer's stream -- a plain copy: the call returns when the bytes have left the caller's memory --,
// launch(at, base, i0, i1, stream) queues the chunk's kernels behind it, and the next chunk's copy runs while they do.  Before a buffer
// is written again its stream is waited for.  with_successor: record i1 is copied behind the chunk.  Returns with both streams idle
template <class Launch>
int staged_pass(const uint8_t *rec, const uint64_t *offs, uint32_t n, const std::vector<uint32_t> &cut, bool with_successor, uint64_t stage_bytes,
                Dev<uint8_t> (&d_stage)[2], TwoStreams &st, Launch &&launch) {
	HIP_TRY(hipStreamSynchronize(nullptr));
	for (size_t c = 0; c + 1 < cut.size(); ++c) {
		const int b = (int)(c & 1u);
		const uint32_t i0 = cut[c], i1 = cut[c + 1], seen = with_successor && i1 < n ? i1 + 1u : i1;
		const uint64_t bytes = offs[seen] - offs[i0];
		if (bytes > stage_bytes) return URMAPX_E_NODEVICE;  // (never: the buffers were sized by these very chunks)
		HIP_TRY(hipStreamSynchronize(st.s[b]));
		if (bytes) HIP_TRY(hipMemcpyAsync(d_stage[b].p, rec + offs[i0], (size_t)bytes, hipMemcpyHostToDevice, st.s[b]));
		if (const int r = launch((const uint8_t *)d_stage[b].p, offs[i0], i0, i1, st.s[b])) return r;
	}
	HIP_TRY(hipGetLastError());
	return st.wait();
}

// What is taken of the records while they pass the device: the depth, the statistics, the pileup.  The planned sort (DeviceSort) and the
// pass on its own (staged_alone) know a by-product by this alone.  An implementation owns its device arrays and knows its result
struct Beside {
	uint64_t *const least_budget;    // in its result
	double *const alloc_s, *const count_s;
	Beside(uint64_t *least_budget_, double *alloc_s_, double *count_s_) : least_budget(least_budget_), alloc_s(alloc_s_), count_s(count_s_) {}
	virtual ~Beside() {}
	virtual uint64_t resident_bytes() const = 0;  // device bytes of begin(): they come off the sort's budget before it is planned
	virtual int begin(uint32_t n) = 0;            // the arrays on the current device, the counters zero; n: the records there are
	// records i0 .. i1 - 1 lie at at + (off[i] - base), as for keys_kernel; action (optional): the marking's decision per record (MD_*),
	// which stands in for bit 0x400.  Queues the counting kernels on `stream`
	virtual int count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) = 0;
	virtual int finish() = 0;                     // once every record is counted: the result
	virtual void free_result() = 0;
};

// The pass on its own (urmapx_bam_depth, urmapx_bam_stats, urmapx_bam_pileup): the chain is scanned, the chunks cut -- a record longer
// than the chunk asked for makes the buffers grow --, B's arrays, the record starts, two staging buffers and the streams allocated in
// that order, the records counted as they pass (*count_s: from the upload of the starts to the streams' end), and B finished
int staged_alone(int device, const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, Beside &B, uint64_t *stage_chunks,
                 double *count_s);

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
