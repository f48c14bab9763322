// bam_sort.hip -- BAM records into coordinate order on the device, with the arrays of their .bai index (urmapx_bam_sort; the
// contract is in include/urmapx.h "Sorted BAM output", what is shared with the host version in bam_sort.h).
//
// The records lie in HBM as they came, back to back, with the start of each (from the host's walk along the block_size chain).
//
//   keys_kernel      one THREAD per record: its packed key (KeyLayout: reference, then position), its number, its end on the reference
//                    (the CIGAR is read byte by byte: a record starts at any address)
//   hist / scatter   one pass of the stable least-significant-digit radix sort of (key, number), 8 bits a pass.  A workgroup owns a
//                    contiguous range of records and walks it 256 at a time.  hist_kernel counts the range's digits; the counts, laid
//                    out digit-major ([digit][workgroup]), go through one exclusive scan and are then each workgroup's first free
//                    place per digit.  scatter_kernel ranks the 64 records of a wavefront among themselves with eight ballots (the
//                    lanes that agree with mine on every bit of the digit; the ones below me are in front of me), the four
//                    wavefronts through their counts in LDS: no atomic decides an order, so equal keys keep their order
//   scan             exclusive prefix sums: a thread sums a contiguous run, one workgroup scans the runs' sums, the threads write
//   gather_kernel    64 records of a slice of the sorted stream per wavefront at a time: every LANE fetches where one of them lies and
//                    goes, then the wavefront copies them one after the other with all its lanes -- the part of the record that lies
//                    in the slice, from any address to any address: bytes up to the destination's next word, whole words, bytes
//   bounds / extent / lin / bin_key / chunk_*   the index: first and last record of every reference and its largest end, the smallest
//                    stream offset per 16 384-base window (atomicMin), a second sort of the record numbers by (reference, bin) with
//                    the same two sort kernels, a flag where a chunk begins, a scan of the flags, the chunks
//   place_fill / place_kernel   the external road (urmapx_bam_sort_external, where the records do not fit the device): only the
//                    per-record arrays are resident, the records pass through two staging buffers in input order -- once for
//                    keys_kernel (and what the marking reads), then once per partition of the sorted stream, where place_kernel
//                    copies the part of every staged record that falls into the partition to its place, as gather_kernel copies
#include "bam_sort_dev.h"
#include "depth_dev.h"
#include "stats_dev.h"
#include "pileup_dev.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <optional>

using namespace urx::bamsort;

namespace {

// (the sizes of the sort's grids -- NT, TILE, MAX_BLOCKS, SCAN_NT, MAX_RUNS -- are in bam_sort_dev.h: markdup.hip sorts with them too;
// the slice, the staged chunk and the bytes per record in bam_sort.h: the plan counts with them on the host)

__device__ __forceinline__ uint32_t load4(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint64_t bcast64(uint64_t v, uint32_t from) {  // lane `from`'s value, in every lane
	return (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)from, 64) << 32 | (uint32_t)__shfl((int)(uint32_t)v, (int)from, 64);
}

// Records i0 .. i1 - 1 lie at rec + (off[i] - base): a staged chunk whose first byte is byte `base` of the input, or (base 0, all
// records) the whole input.  flag4[i]: does the record carry flag 0x4 -- all bounds_kernel wants of a record's bytes
__global__ __launch_bounds__(NT) void keys_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, KeyLayout K, uint64_t *key,
                                                  uint32_t *val, uint32_t *end, uint32_t *flag4) {
	for (uint64_t i = (uint64_t)i0 + blockIdx.x * NT + threadIdx.x; i < i1; i += gridDim.x * NT) {
		const uint8_t *r = rec + (off[i] - base);
		const uint32_t ref_id = load_u32(r + 4), pos = load_u32(r + 8);
		key[i] = K.key(ref_id, pos);
		val[i] = (uint32_t)i;
		end[i] = ref_id == 0xFFFFFFFFu ? 0u : (uint32_t)ref_end(r, (uint32_t)(off[i + 1] - off[i]), pos);
		flag4[i] = load_u32(r + 16) >> 16 & 4u;
	}
}

// ---- one radix pass ----
// workgroup b owns records [b * per_block, min(n, (b + 1) * per_block)); per_block is a multiple of NT
__global__ __launch_bounds__(NT) void hist_kernel(const uint64_t *key, uint32_t n, uint32_t shift, uint32_t per_block, uint32_t *hist) {
	__shared__ uint32_t h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
	for (uint64_t i = lo + threadIdx.x; i < hi; i += NT) atomicAdd(&h[(uint32_t)(key[i] >> shift) & 255u], 1u);
	__syncthreads();
	hist[threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(NT) void scatter_kernel(const uint64_t *key_in, const uint32_t *val_in, uint64_t *key_out, uint32_t *val_out, uint32_t n,
                                                     uint32_t shift, uint32_t per_block, const uint32_t *first) {
	__shared__ uint32_t s_next[256];     // next free place of every digit for this workgroup
	__shared__ uint32_t s_count[4][256]; // this round: records of a digit in each wavefront
	const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
	s_next[t] = first[t * gridDim.x + blockIdx.x];
	for (int k = 0; k < 4; ++k) s_count[k][t] = 0;
	__syncthreads();
	const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
	for (uint64_t base = lo; base < hi; base += NT) {  // (the same trips for every thread: there are barriers inside)
		const uint64_t i = base + t;
		const bool on = i < hi;
		const uint64_t k = on ? key_in[i] : 0;
		const uint32_t v = on ? val_in[i] : 0;
		const uint32_t d = (uint32_t)(k >> shift) & 255u;
		uint64_t same = __ballot(on);
#pragma unroll
		for (uint32_t bit = 0; bit < 8u; ++bit) {
			const bool mine = (d >> bit) & 1u;
			const uint64_t set = __ballot(mine);
			same &= mine ? set : ~set;
		}
		const uint32_t rank = (uint32_t)__popcll(same & (((uint64_t)1 << lane) - 1u));
		if (on && rank == 0) s_count[w][d] = (uint32_t)__popcll(same);
		__syncthreads();
		if (on) {
			uint32_t at = s_next[d] + rank;
			for (uint32_t k2 = 0; k2 < w; ++k2) at += s_count[k2][d];
			if (at < n) { key_out[at] = k; val_out[at] = v; }  // (always: the places are hist_kernel's counts of these very records)
		}
		__syncthreads();
		s_next[t] += s_count[0][t] + s_count[1][t] + s_count[2][t] + s_count[3][t];
		for (int k2 = 0; k2 < 4; ++k2) s_count[k2][t] = 0;
		__syncthreads();
	}
}

// ---- exclusive scans ----
// one workgroup: out[i] = in[0] + .. + in[i - 1] for i < m (out may be in), the total to out[m] if with_total
template <class TI, class TO>
__global__ __launch_bounds__(SCAN_NT) void scan_block_kernel(const TI *in, TO *out, uint32_t m, int with_total) {
	__shared__ uint64_t part[SCAN_NT];
	const uint32_t t = threadIdx.x, run = (m + SCAN_NT - 1) / SCAN_NT;
	const uint64_t lo = (uint64_t)t * run < m ? (uint64_t)t * run : m, hi = lo + run < m ? lo + run : m;
	uint64_t sum = 0;
	for (uint64_t i = lo; i < hi; ++i) sum += in[i];
	part[t] = sum;
	__syncthreads();
	for (uint32_t s = 1; s < SCAN_NT; s <<= 1) {
		const uint64_t a = t >= s ? part[t - s] : 0;
		__syncthreads();
		part[t] += a;
		__syncthreads();
	}
	uint64_t at = part[t] - sum;
	for (uint64_t i = lo; i < hi; ++i) {
		const uint64_t x = in[i];
		out[i] = (TO)at;
		at += x;
	}
	if (with_total && t == SCAN_NT - 1) out[m] = (TO)part[t];
}
// n values in runs of `run`: the runs' sums
template <class TI>
__global__ __launch_bounds__(NT) void scan_sums_kernel(const TI *in, uint32_t n, uint32_t run, uint32_t n_runs, uint64_t *sums) {
	const uint32_t g = blockIdx.x * NT + threadIdx.x;
	if (g >= n_runs) return;
	const uint64_t lo = (uint64_t)g * run, hi = lo + run < n ? lo + run : n;
	uint64_t sum = 0;
	for (uint64_t i = lo; i < hi; ++i) sum += in[i];
	sums[g] = sum;
}
// the scanned sums back onto the runs; out[n] = the total (out is not in)
template <class TI, class TO>
__global__ __launch_bounds__(NT) void scan_write_kernel(const TI *in, uint32_t n, uint32_t run, uint32_t n_runs, const uint64_t *sums, TO *out) {
	const uint32_t g = blockIdx.x * NT + threadIdx.x;
	if (g >= n_runs) return;
	const uint64_t lo = (uint64_t)g * run, hi = lo + run < n ? lo + run : n;
	uint64_t at = sums[g];
	for (uint64_t i = lo; i < hi; ++i) {
		out[i] = (TO)at;
		at += in[i];
	}
	if (g == n_runs - 1) out[n] = (TO)at;
}

// ---- the sorted stream ----
__global__ __launch_bounds__(NT) void sorted_len_kernel(const uint32_t *val, const uint64_t *off, uint32_t n, uint32_t *len) {
	for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < n; k += gridDim.x * NT) len[k] = (uint32_t)(off[val[k] + 1] - off[val[k]]);
}

// the sorted records that have a byte in [s0, s1) of the stream: range[0] .. range[1] - 1.  One thread.
__global__ void slice_range_kernel(const uint64_t *dst, uint32_t n, uint64_t s0, uint64_t s1, uint32_t *range) {
	uint32_t a = 0, b = n;  // first k whose end dst[k + 1] lies behind s0
	while (a < b) {
		const uint32_t m = a + (b - a) / 2;
		if (dst[m + 1] > s0) b = m; else a = m + 1;
	}
	range[0] = a;
	b = n;  // first k at or behind a that starts at or behind s1
	while (a < b) {
		const uint32_t m = a + (b - a) / 2;
		if (dst[m] >= s1) b = m; else a = m + 1;
	}
	range[1] = a;
}

__global__ __launch_bounds__(NT) void gather_kernel(const uint8_t *rec, const uint64_t *off, const uint32_t *val, const uint64_t *dst, const uint32_t *range,
                                                    uint64_t s0, uint64_t s1, uint8_t *out) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t wave = ((uint64_t)blockIdx.x * NT + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (NT / 64);
	const uint64_t k1 = range[1];
	// 64 records at a time: every LANE fetches where one of them lies and goes (three dependent loads, once for the 64), then the
	// wavefront copies them one after the other with all its lanes
	for (uint64_t base = range[0] + wave * 64u; base < k1; base += n_waves * 64u) {
		const uint64_t k = base + lane;
		uint64_t my_d0 = 0, my_d1 = 0, my_src = 0;
		if (k < k1) { my_d0 = dst[k]; my_d1 = dst[k + 1]; my_src = off[val[k]]; }
		const uint32_t cnt = (uint32_t)(k1 - base < 64u ? k1 - base : 64u);
		for (uint32_t t = 0; t < cnt; ++t) {
			const uint64_t d0 = bcast64(my_d0, t), d1 = bcast64(my_d1, t);
			const uint64_t lo = d0 > s0 ? d0 : s0, hi = d1 < s1 ? d1 : s1;  // a record may begin in front of the slice or end behind it
			if (hi <= lo) continue;
			const uint8_t *src = rec + bcast64(my_src, t) + (lo - d0);
			uint8_t *to = out + (lo - s0);
			const uint32_t len = (uint32_t)(hi - lo);
			const uint32_t to_word = (uint32_t)((4u - ((uintptr_t)to & 3u)) & 3u), head = len < to_word ? len : to_word;
			if (lane < head) to[lane] = src[lane];
			const uint32_t words = (len - head) >> 2;
			uint32_t *tw = (uint32_t *)(to + head);
			const uint8_t *sw = src + head;
			for (uint32_t i = lane; i < words; i += 64u) tw[i] = load4(sw + 4u * i);
			const uint32_t done = head + 4u * words;
			if (lane < len - done) to[done + lane] = src[done + lane];
		}
	}
}

// ---- the external road: the records are not resident, they pass through a staging buffer in input order ----
// where every record of the input goes in the sorted stream
__global__ __launch_bounds__(NT) void place_fill_kernel(const uint32_t *val, const uint64_t *dst, uint32_t n, uint64_t *place) {
	for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < n; k += gridDim.x * NT) place[val[k]] = dst[k];
}

// Records i0 .. i1 - 1 lie in `stage` from byte `base` of the input on; `part` is the partition [s0, s1) of the sorted stream.  As in
// gather_kernel a wavefront takes 64 records at a time, every LANE fetching where one of them goes, how long it is and what becomes of
// its bit 0x400; then the wavefront copies, with all lanes, the part of each that lies inside the partition -- a record may begin in
// front of it, end behind it or cover it whole -- in gather_kernel's form: bytes up to the destination's next word, whole words from
// an unaligned source, bytes.  A record outside the partition is dropped on what the lanes fetched: its bytes are not read.  Byte 19
// of a record (FLAG_BYTE) takes its bit from the action in the one lane that copies it, in whichever partition holds that byte.
__global__ __launch_bounds__(NT) void place_kernel(const uint8_t *stage, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint64_t *place,
                                                   const uint8_t *action, uint64_t s0, uint64_t s1, uint8_t *part) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t wave = ((uint64_t)blockIdx.x * NT + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (NT / 64);
	for (uint64_t first = i0 + wave * 64u; first < i1; first += n_waves * 64u) {
		const uint64_t i = first + lane;
		uint64_t my_d0 = 0, my_src = 0;
		uint32_t my_len = 0, my_act = MD_KEEP;
		if (i < i1) {
			my_d0 = place[i];
			my_src = off[i] - base;
			my_len = (uint32_t)(off[i + 1] - off[i]);
			if (action) my_act = action[i];
		}
		const uint32_t cnt = (uint32_t)(i1 - first < 64u ? i1 - first : 64u);
		for (uint32_t t = 0; t < cnt; ++t) {
			const uint64_t d0 = bcast64(my_d0, t), d1 = d0 + (uint32_t)__shfl((int)my_len, (int)t, 64);
			const uint64_t lo = d0 > s0 ? d0 : s0, hi = d1 < s1 ? d1 : s1;
			if (hi <= lo) continue;  // (the same in all lanes)
			const uint32_t act = (uint32_t)__shfl((int)my_act, (int)t, 64);
			const uint8_t *src = stage + bcast64(my_src, t) + (lo - d0);
			uint8_t *to = part + (lo - s0);
			const uint32_t len = (uint32_t)(hi - lo);
			// the flag byte's place among the bytes copied here; none: beyond every index
			const uint64_t fb64 = d0 + FLAG_BYTE;
			const uint32_t fb = act != MD_KEEP && fb64 >= lo && fb64 < hi ? (uint32_t)(fb64 - lo) : 0xFFFFFFFFu;
			const uint32_t set = act == MD_SET ? FLAG_DUP_BIT : 0u;
			const uint32_t to_word = (uint32_t)((4u - ((uintptr_t)to & 3u)) & 3u), head = len < to_word ? len : to_word;
			if (lane < head) {
				const uint32_t b = src[lane];
				to[lane] = (uint8_t)(lane == fb ? (b & ~(uint32_t)FLAG_DUP_BIT) | set : b);
			}
			const uint32_t words = (len - head) >> 2;
			uint32_t *tw = (uint32_t *)(to + head);
			const uint8_t *sw = src + head;
			const uint32_t fw = fb != 0xFFFFFFFFu && fb >= head ? (fb - head) >> 2 : 0xFFFFFFFFu, fs = 8u * ((fb - head) & 3u);
			for (uint32_t w = lane; w < words; w += 64u) {
				uint32_t v = load4(sw + 4u * w);
				if (w == fw) v = (v & ~((uint32_t)FLAG_DUP_BIT << fs)) | set << fs;
				tw[w] = v;
			}
			const uint32_t done = head + 4u * words;
			if (lane < len - done) {
				const uint32_t b = src[done + lane];
				to[done + lane] = (uint8_t)(done + lane == fb ? (b & ~(uint32_t)FLAG_DUP_BIT) | set : b);
			}
		}
	}
}

// ---- the index ----
// per sorted record: where its reference's records begin and end; the reference's largest end (one atomic per wavefront where its 64
// records share the reference, which in sorted order is nearly everywhere); its records with flag 4 (has4[i]: keys_kernel's note of
// record i, so no record's bytes are read here).  The largest end is that of the index (bam_sort.h INDEX_END): a record that begins
// beyond counts for nothing, one that ends beyond for 2^29
__global__ __launch_bounds__(NT) void bounds_kernel(const uint32_t *has4, const uint64_t *key, const uint32_t *val, const uint32_t *end,
                                                    uint32_t n, KeyLayout K, uint32_t *first, uint32_t *last, uint32_t *max_end, uint32_t *flag4) {
	const uint32_t rounds = (n + gridDim.x * NT - 1) / (gridDim.x * NT);
	for (uint32_t it = 0; it < rounds; ++it) {  // (whole wavefronts stay together for the shuffles)
		const uint32_t k = (it * gridDim.x + blockIdx.x) * NT + threadIdx.x;
		const bool on = k < n;
		const uint32_t r = on ? K.ref_of(key[k]) : 0xFFFFFFFFu;
		uint32_t e = 0;
		if (on) {
			if (k == 0 || K.ref_of(key[k - 1]) != r) first[r] = k;
			if (k == n - 1 || K.ref_of(key[k + 1]) != r) last[r] = k;
			if (r < K.n_ref) {
				e = indexed(K.pos_of(key[k])) ? (uint32_t)index_end(end[val[k]]) : 0u;
				if (has4[val[k]]) atomicAdd(&flag4[r], 1u);
			}
		}
		const uint32_t r0 = __shfl(r, 0, 64);
		if (__all(r == r0)) {
			for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(e, d, 64); e = o > e ? o : e; }
			if ((threadIdx.x & 63) == 0 && r0 < K.n_ref) atomicMax(&max_end[r0], e);
		} else if (on && r < K.n_ref) atomicMax(&max_end[r], e);
	}
}
__global__ __launch_bounds__(NT) void extent_kernel(const uint32_t *first, const uint32_t *last, const uint64_t *dst, uint32_t n_ref1, uint64_t *beg, uint64_t *end) {
	const uint32_t r = blockIdx.x * NT + threadIdx.x;
	if (r >= n_ref1) return;
	const bool any = first[r] != 0xFFFFFFFFu;
	beg[r] = any ? dst[first[r]] : 0;
	end[r] = any ? dst[last[r] + 1] : 0;
}
__global__ __launch_bounds__(NT) void lin_kernel(const uint64_t *key, const uint32_t *val, const uint32_t *end, const uint64_t *dst, uint32_t m, KeyLayout K,
                                                 const uint64_t *win_base, unsigned long long *lin) {
	for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < m; k += gridDim.x * NT) {
		const uint32_t r = K.ref_of(key[k]);
		const uint64_t w0 = win_base[r], n_win = win_base[r + 1] - w0;
		const uint64_t pos = K.pos_of(key[k]);
		if (!indexed(pos)) continue;
		const uint64_t a = pos >> WINDOW_SHIFT, b = (index_end(end[val[k]]) - 1u) >> WINDOW_SHIFT;
		for (uint64_t w = a; w <= b && w < n_win; ++w) atomicMin(&lin[w0 + w], (unsigned long long)dst[k]);
	}
}
// (a record beyond the index gets NO_BIN: the second sort puts it behind its reference's bins, and no chunk is made of it)
__global__ __launch_bounds__(NT) void bin_key_kernel(const uint64_t *key, const uint32_t *val, const uint32_t *end, uint32_t m, KeyLayout K, uint64_t *key2,
                                                     uint32_t *val2) {
	for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < m; k += gridDim.x * NT) {
		const uint64_t pos = K.pos_of(key[k]);
		key2[k] = (uint64_t)K.ref_of(key[k]) << BIN_BITS | (indexed(pos) ? reg2bin(pos, index_end(end[val[k]])) : NO_BIN);
		val2[k] = k;
	}
}
__device__ __forceinline__ bool no_bin(uint64_t key2) { return (key2 & NO_BIN) == NO_BIN; }
// a chunk begins where the (reference, bin) changes or the record is not the file's next one; none at a record without a bin
__global__ __launch_bounds__(NT) void chunk_flag_kernel(const uint64_t *key2, const uint32_t *val2, uint32_t m, uint32_t *flag) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < m; j += gridDim.x * NT)
		flag[j] = !no_bin(key2[j]) && (j == 0 || key2[j] != key2[j - 1] || val2[j] != val2[j - 1] + 1u);
}
__global__ __launch_bounds__(NT) void chunk_write_kernel(const uint64_t *key2, const uint32_t *val2, const uint32_t *flag, const uint32_t *index, const uint64_t *dst,
                                                         uint32_t m, uint32_t n_chunks, Chunk *chunks) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < m; j += gridDim.x * NT) {
		if (no_bin(key2[j])) continue;
		const uint32_t c = index[j] + flag[j] - 1u;  // (index: chunks that begin in front of j)
		if (c >= n_chunks) continue;
		if (flag[j]) {
			chunks[c].ref = (uint32_t)(key2[j] >> BIN_BITS);
			chunks[c].bin = (uint32_t)(key2[j] & NO_BIN);
			chunks[c].beg = dst[val2[j]];
		}
		if (j == m - 1 || flag[j + 1] || no_bin(key2[j + 1])) chunks[c].end = dst[val2[j] + 1];
	}
}

// ---- host side ----
using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

}  // namespace

// ---- what markdup.hip uses too (declared in bam_sort_dev.h) ----
namespace urx {
namespace bamsort {

thread_local double t_alloc_s = 0;

// out[0 .. n] = exclusive sums of in[0 .. n), the total in out[n]; sums: MAX_RUNS + 1 entries of scratch
template <class TI, class TO>
void scan_launch(const TI *in, uint32_t n, TO *out, uint64_t *sums) {
	uint32_t run = (n + MAX_RUNS - 1) / MAX_RUNS;
	if (run < 16) run = 16;
	const uint32_t n_runs = (n + run - 1) / run;
	if (n_runs == 0) { hipLaunchKernelGGL((scan_block_kernel<TI, TO>), dim3(1), dim3(SCAN_NT), 0, nullptr, in, out, 0u, 1); return; }
	hipLaunchKernelGGL((scan_sums_kernel<TI>), dim3(grid_for(n_runs)), dim3(NT), 0, nullptr, in, n, run, n_runs, sums);
	hipLaunchKernelGGL((scan_block_kernel<uint64_t, uint64_t>), dim3(1), dim3(SCAN_NT), 0, nullptr, (const uint64_t *)sums, sums, n_runs, 0);
	hipLaunchKernelGGL((scan_write_kernel<TI, TO>), dim3(grid_for(n_runs)), dim3(NT), 0, nullptr, in, n, run, n_runs, (const uint64_t *)sums, out);
}

// stable sort of (key, val)[0 .. n) by the low `bits` bits of the key, between two pairs of arrays; `in` says where the result is
uint32_t radix_sort(SortArrays &S, uint32_t n, uint32_t bits, uint32_t *hist) {
	if (n == 0) return 0;
	const uint32_t tiles = (n + TILE - 1) / TILE, blocks = tiles < MAX_BLOCKS ? tiles : MAX_BLOCKS;
	const uint32_t per_block = (tiles + blocks - 1) / blocks * TILE;
	uint32_t passes = 0;
	for (uint32_t shift = 0; shift < bits; shift += 8, ++passes) {
		const int a = S.in, b = 1 - S.in;
		hipLaunchKernelGGL(hist_kernel, dim3(blocks), dim3(NT), 0, nullptr, (const uint64_t *)S.key[a], n, shift, per_block, hist);
		hipLaunchKernelGGL((scan_block_kernel<uint32_t, uint32_t>), dim3(1), dim3(SCAN_NT), 0, nullptr, (const uint32_t *)hist, hist, 256u * blocks, 0);
		hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(NT), 0, nullptr, (const uint64_t *)S.key[a], (const uint32_t *)S.val[a], S.key[b], S.val[b], n, shift,
		                   per_block, (const uint32_t *)hist);
		S.in = b;
	}
	return passes;
}
template void scan_launch<uint32_t, uint64_t>(const uint32_t *, uint32_t, uint64_t *, uint64_t *);
template void scan_launch<uint32_t, uint32_t>(const uint32_t *, uint32_t, uint32_t *, uint64_t *);

int staged_alone(int device, const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, Beside &B, uint64_t *stage_chunks,
                 double *count_s) {
	std::vector<uint64_t> offs;
	int rc = urx::depth::scan_for_depth(rec, n_bytes, n_ref, starts, n_starts, offs);
	if (rc) return rc;
	const uint32_t n = (uint32_t)(offs.size() - 1);
	std::vector<uint32_t> cut;
	uint64_t stage = default_stage_bytes(n_bytes);
	stage = std::max(stage, cut_chunks(offs.data(), n, stage, false, cut));
	*stage_chunks = cut.size() - 1;

	HIP_TRY(hipSetDevice(device));
	Dev<uint64_t> d_off;
	Dev<uint8_t> d_stage[2];
	TwoStreams st;
	// (the pieces the by-products' standalone_bytes count, in their order)
	if ((rc = B.begin(n)) || (rc = d_off.alloc((size_t)n + 1)) || (rc = d_stage[0].alloc((size_t)stage + 16)) || (rc = d_stage[1].alloc((size_t)stage + 16)) ||
	    (rc = st.create()))
		return rc;
	const auto t = Clock::now();
	HIP_TRY(hipMemcpy(d_off.p, offs.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
	rc = staged_pass(rec, offs.data(), n, cut, false, stage, d_stage, st, [&](const uint8_t *at, uint64_t base, uint32_t i0, uint32_t i1, hipStream_t s) {
		return B.count(at, base, d_off.p, i0, i1, nullptr, s);
	});
	if (rc) return rc;
	*count_s = since(t);
	return B.finish();
}

}  // namespace bamsort
}  // namespace urx

namespace {

// adds the time from where it is made to the end of its scope
struct Span {
	double &to;
	const Clock::time_point t0 = Clock::now();
	explicit Span(double &sum) : to(sum) {}
	~Span() { to += since(t0); }
};
struct BgzfDestroy { void operator()(urmapx_bgzf *z) const { urmapx_bgzf_destroy(z); } };
struct Free { void operator()(void *p) const { free(p); } };
struct KeyVal { uint64_t *key; uint32_t *val; };  // a key array and the record-number array that moves with it
struct ChunkMarks { uint32_t *flag, *index; };    // per placed record: does a chunk begin here; behind the flags their sums, one more

// One device sort, from the caller's records to the result.  budget == nullptr: the in-core road, whatever it takes (urmapx_bam_sort,
// urmapx_bam_sort_markdup).  Else the road the plan names for *budget device bytes (urmapx_bam_sort_external), with `beside` for what
// their arrays leave of them (urmapx_bam_sort_with).  run() lists the stages; a stage returns a code, and the first that is not 0 ends
// the run: every member lets go of what it holds.
struct DeviceSort {
	// ---- what the caller gave (sort_entry) ----
	const int device;
	const uint64_t *const budget;
	const uint8_t *const rec;
	const size_t n_bytes;
	const uint32_t n_ref;
	const uint64_t in_front;
	const uint64_t *const starts;
	const size_t n_starts;
	urmapx_markdup_stats *const md;
	const std::vector<Beside *> &beside;  // what is taken on the way, in the order depth, statistics, pileup
	urmapx_bam_sort_result *const out;
	size_t n_ref1() const { return (size_t)n_ref + 1; }
	bool look() const { return md != nullptr; }  // the marking compares neighbours: a staged chunk is followed by its successor

	// ---- what the scan gives ----
	std::vector<uint64_t> offs;
	uint32_t n = 0;
	KeyLayout K;

	// ---- the road; on the external one the staged chunks: chunk c is records cut[c] .. cut[c + 1] - 1 ----
	urmapx_bam_sort_plan P{};
	std::vector<uint32_t> cut;
	bool ext = false;
	uint64_t beside_bytes = 0, sort_budget = 0;

	// ---- the device arrays, in the order they are allocated (external_device_bytes counts them in this order) ----
	// What each holds, stage by stage; "free" means any later stage may take it.
	//                    keys+sort        destinations   index arrays                      marking       stream
	//   d_rec (in core)  records          .              .                                 bit 0x400     gather reads
	//   d_off            starts           read           .                                 read          read
	//   d_key[0], [1]    keys, ping-pong  .              by_coor.key read; then the        key[0], [1]   spare.key = place (external)
	//                    -> by_coor.key,                 second sort's keys, and flag and
	//                       spare.key                    index in the one it leaves free
	//   d_val[0], [1]    numbers          spare.val =    by_coor.val read; spare.val the   spare.val =   by_coor.val read
	//                    -> by_coor.val,  lengths        second sort's other numbers       val[0]
	//                       spare.val
	//   d_val[2]         notes4           .              notes4 read (bounds_kernel);      val[1]        free
	//                                                    then the second sort's numbers
	//   d_end            ends             .              read (lin, bin_key)               score         free
	//   d_dst            .                written        read                              .             read
	//   d_hist, d_sums   scratch of every sort and scan, the marking's too
	//   d_ref, d_ext, d_win, d_lin, d_chunks   the index arrays' own, read back by the index stage
	//   d_stage, d_part, d_action (external)   staging buffers: both passes; the partition: stream; the decisions: marking -> stream
	Dev<uint8_t> d_rec, d_stage[2], d_part, d_action;
	Dev<uint64_t> d_off, d_dst, d_key[2], d_sums, d_ext[2], d_win, d_lin;
	Dev<uint32_t> d_val[3], d_end, d_hist, d_range, d_ref[4];
	Dev<Chunk> d_chunks;
	MarkdupOwn W;
	TwoStreams st;
	IndexArrays X;
	// ---- the arrays' later names; each is given in one place ----
	uint32_t *notes4 = nullptr;  // does record i carry flag 0x4: from keys_kernel to bounds_kernel
	KeyVal by_coor{}, spare{};   // after the coordinate sort: the sorted keys and record numbers, and the pair the sort left free
	uint32_t *lengths = nullptr; // the records' lengths in sorted order
	uint64_t *place = nullptr;   // external road: where record i of the input goes in the sorted stream
	Clock::time_point t_sort;    // where sort_s begins

	// ---- the sorted stream: a slice, its members, the compressor, the members on the host ----
	size_t slice_bytes = 0, z_cap = 0, host_cap = 0, z_bytes = 0;
	Dev<uint8_t> d_slice, d_z;
	Dev<uint64_t> d_used;
	std::unique_ptr<urmapx_bgzf, BgzfDestroy> Z;
	std::unique_ptr<uint8_t, Free> z;

	int run() {
		int rc;
		if ((rc = scan_chain()) || (rc = choose_road()) || (rc = allocate()) || (rc = upload()) || (rc = sort_by_coordinate()) || (rc = destinations()) ||
		    (rc = index_arrays()) || (rc = mark_duplicates()) || (rc = beside_in_core()) || (rc = sorted_stream()))
			return rc;
		return finish();
	}

	int scan_chain() {
		uint32_t max_pos = 0;
		{
			Span span(out->scan_s);
			if (const int rc = scan_records(rec, n_bytes, n_ref, starts, n_starts, offs, max_pos)) return rc;
		}
		n = (uint32_t)(offs.size() - 1);
		out->records = n;
		K = key_layout(n_ref, max_pos);
		return URMAPX_OK;
	}

	// the plan for staged chunks of `stage` bytes; where nothing fits, the least budget is the by-products' arrays' and the plan's
	int plan(uint64_t stage) {
		const int r = plan_with_stage(n_bytes, n, md != nullptr, sort_budget, stage, &P);
		if (r == URMAPX_E_NOMEM)
			for (Beside *B : beside) *B->least_budget = beside_bytes + P.device_bytes;
		return r;
	}
	// The road.  On the external one the staged chunks, under marking each with the next chunk's first record behind it (first_kernel
	// compares neighbours).  A staging buffer holds the largest of them: a record longer than the staged chunk asked for, or its
	// successor, makes the buffers grow, and the partition is planned again around them
	int choose_road() {
		if (budget) {
			// the by-products' arrays come off the budget before the sort is planned
			for (const Beside *B : beside) beside_bytes += B->resident_bytes();
			sort_budget = *budget > beside_bytes ? *budget - beside_bytes : 0u;
			if (const int rc = plan(default_stage_bytes(n_bytes))) return rc;
			if (P.external) {
				const uint64_t need = cut_chunks(offs.data(), n, P.stage_bytes, look(), cut);
				if (need > P.stage_bytes)
					if (const int rc = plan(need)) return rc;
			}
		}
		ext = P.external != 0;
		out->external = ext;
		out->partitions = (uint32_t)P.partitions;
		out->stage_chunks = ext ? cut.size() - 1 : 0;
		return URMAPX_OK;
	}

	int allocate() {
		int rc;
		HIP_TRY(hipSetDevice(device));
		if (!beside.empty() && n >= 0x7FFFFFFFu) return URMAPX_E_ARG;
		for (Beside *B : beside) {
			const double a0 = t_alloc_s;
			if ((rc = B->begin(n))) return rc;
			*B->alloc_s = t_alloc_s - a0;
		}
		if (ext) {  // (the pieces external_device_bytes counts, in its order; the partition is not larger than the stream)
			const size_t part_cap = (size_t)std::min<uint64_t>(P.partition_bytes, n_bytes);
			if ((md && ((rc = W.begin(n)) || (rc = d_action.alloc(n)))) || (rc = d_stage[0].alloc((size_t)P.stage_bytes + 16)) ||
			    (rc = d_stage[1].alloc((size_t)P.stage_bytes + 16)) || (rc = d_part.alloc(part_cap + 16)) || (rc = st.create()))
				return rc;
			if (md) HIP_TRY(hipMemset(d_action.p, MD_KEEP, n ? n : 1));
		} else if ((rc = d_rec.alloc(n_bytes + 16)))
			return rc;
		if ((rc = d_off.alloc((size_t)n + 1)) || (rc = d_dst.alloc((size_t)n + 1)) || (rc = d_key[0].alloc((size_t)n + 2)) ||
		    (rc = d_key[1].alloc((size_t)n + 2)) || (rc = d_val[0].alloc((size_t)n + 1)) || (rc = d_val[1].alloc((size_t)n + 1)) ||
		    (rc = d_val[2].alloc((size_t)n + 1)) || (rc = d_end.alloc(n)) || (rc = d_hist.alloc((size_t)256 * MAX_BLOCKS)) || (rc = d_sums.alloc(MAX_RUNS + 1)) ||
		    (rc = d_range.alloc(2)) || (rc = d_ext[0].alloc(n_ref1())) || (rc = d_ext[1].alloc(n_ref1())) || (rc = d_win.alloc(n_ref1() + 1)))
			return rc;
		for (int k = 0; k < 4; ++k)
			if ((rc = d_ref[k].alloc(n_ref1()))) return rc;
		return URMAPX_OK;
	}

	int upload() {
		Span span(out->upload_s);
		if (!ext && n_bytes) HIP_TRY(hipMemcpy(d_rec.p, rec, n_bytes, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_off.p, offs.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		return URMAPX_OK;
	}

	// one pass over the input on the external road (staged_pass): its time counts in stage_s
	template <class Launch>
	int pass(bool with_successor, Launch &&launch) {
		const auto t0 = Clock::now();
		const int r = staged_pass(rec, offs.data(), n, cut, with_successor, P.stage_bytes, d_stage, st, launch);
		out->stage_s += since(t0);
		return r;
	}

	// keys, numbers, ends and notes of records i0 .. i1 - 1 at `at`; on the external road what the marking reads of them, as they pass
	int keys_of(const uint8_t *at, uint64_t base, uint32_t i0, uint32_t i1, hipStream_t s) {
		hipLaunchKernelGGL(keys_kernel, dim3(grid_for(i1 - i0)), dim3(NT), 0, s, at, base, d_off.p, i0, i1, K, d_key[0].p, d_val[0].p, d_end.p, notes4);
		return md && ext ? markdup_chunk(W, at, base, d_off.p, i0, i1, n, s) : URMAPX_OK;
	}
	// Keys and the coordinate sort.  On the external road the keys are the first pass, which counts in stage_s and not in sort_s
	int sort_by_coordinate() {
		notes4 = d_val[2].p;  // (free until the second sort)
		if (ext)
			if (const int rc = pass(look(), [this](const uint8_t *at, uint64_t base, uint32_t i0, uint32_t i1, hipStream_t s) { return keys_of(at, base, i0, i1, s); })) return rc;
		t_sort = Clock::now();
		if (!ext && n) (void)keys_of(d_rec.p, 0, 0, n, nullptr);
		SortArrays S{{d_key[0].p, d_key[1].p}, {d_val[0].p, d_val[1].p}, 0};
		out->sort_passes = radix_sort(S, n, K.bits(), d_hist.p);
		by_coor = KeyVal{S.key[S.in], S.val[S.in]};
		spare = KeyVal{S.key[1 - S.in], S.val[1 - S.in]};  // (the sort's last pass read it: nothing in it is wanted any more)
		return URMAPX_OK;
	}

	// where every sorted record goes: the lengths in sorted order, scanned
	int destinations() {
		lengths = spare.val;
		if (n) hipLaunchKernelGGL(sorted_len_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, by_coor.val, d_off.p, n, lengths);
		scan_launch<uint32_t, uint64_t>(lengths, n, d_dst.p, d_sums.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(nullptr));
		out->sort_s = since(t_sort);
		return URMAPX_OK;
	}

	int index_arrays() {
		Span span(out->index_s);
		if (const int rc = index_references()) return rc;
		return index_bins();
	}
	// per reference: its first and last sorted record, its extent in the stream, its counts, its windows
	int index_references() {
		X.refs.assign(n_ref, RefExtent());
		X.win_base.assign(n_ref1(), 0);
		std::vector<uint32_t> first(n_ref1(), 0xFFFFFFFFu), last(n_ref1(), 0), max_end(n_ref1(), 0), flag4(n_ref1(), 0);
		std::vector<uint64_t> ext_beg(n_ref1(), 0), ext_end(n_ref1(), 0);
		HIP_TRY(hipMemset(d_ref[0].p, 0xFF, n_ref1() * 4));
		for (int k = 1; k < 4; ++k) HIP_TRY(hipMemset(d_ref[k].p, 0, n_ref1() * 4));
		if (n) {
			hipLaunchKernelGGL(bounds_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, notes4, by_coor.key, by_coor.val, d_end.p, n, K, d_ref[0].p, d_ref[1].p,
			                   d_ref[2].p, d_ref[3].p);
			hipLaunchKernelGGL(extent_kernel, dim3(grid_for(n_ref1(), 1u << 22)), dim3(NT), 0, nullptr, d_ref[0].p, d_ref[1].p, d_dst.p, (uint32_t)n_ref1(), d_ext[0].p,
			                   d_ext[1].p);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpy(first.data(), d_ref[0].p, n_ref1() * 4, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(last.data(), d_ref[1].p, n_ref1() * 4, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(max_end.data(), d_ref[2].p, n_ref1() * 4, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(flag4.data(), d_ref[3].p, n_ref1() * 4, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ext_beg.data(), d_ext[0].p, n_ref1() * 8, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(ext_end.data(), d_ext[1].p, n_ref1() * 8, hipMemcpyDeviceToHost));
		}
		for (uint32_t r = 0; r < n_ref; ++r) {
			if (first[r] != 0xFFFFFFFFu) {
				const uint64_t cnt = (uint64_t)last[r] - first[r] + 1u;
				X.refs[r].beg = ext_beg[r]; X.refs[r].end = ext_end[r];
				X.refs[r].n_unmapped = flag4[r]; X.refs[r].n_mapped = cnt - flag4[r];
			}
			X.win_base[r + 1] = X.win_base[r] + (max_end[r] ? (((uint64_t)max_end[r] - 1u) >> WINDOW_SHIFT) + 1u : 0u);
		}
		X.n_no_coor = first[n_ref] != 0xFFFFFFFFu ? (uint64_t)last[n_ref] - first[n_ref] + 1u : 0u;
		out->no_coor = X.n_no_coor;
		return URMAPX_OK;
	}
	// the linear index, then the chunks: the placed records' numbers sorted by (reference, bin), a flag where a chunk begins, the flags
	// scanned.  (d_lin and d_chunks are allocated here, where their sizes are known)
	int index_bins() {
		const uint32_t m = n - (uint32_t)X.n_no_coor;  // the placed records: the first m of the sorted ones
		const size_t n_win = (size_t)X.win_base[n_ref];
		X.lin.assign(n_win, NONE);
		if (!m) return URMAPX_OK;
		int rc;
		if ((rc = d_lin.alloc(n_win))) return rc;
		HIP_TRY(hipMemset(d_lin.p, 0xFF, n_win * 8));
		HIP_TRY(hipMemcpy(d_win.p, X.win_base.data(), n_ref1() * 8, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(lin_kernel, dim3(grid_for(m)), dim3(NT), 0, nullptr, by_coor.key, by_coor.val, d_end.p, d_dst.p, m, K, d_win.p, (unsigned long long *)d_lin.p);
		// The second sort runs between the two key arrays: bin_key_kernel is the last reader of the coordinate keys.  Its numbers go to
		// d_val[2] (the notes: bounds_kernel has read them) and the lengths (scanned into d_dst by destinations); by_coor.val stays
		SortArrays S2{{spare.key, by_coor.key}, {d_val[2].p, lengths}, 0};
		hipLaunchKernelGGL(bin_key_kernel, dim3(grid_for(m)), dim3(NT), 0, nullptr, by_coor.key, by_coor.val, d_end.p, m, K, S2.key[0], S2.val[0]);
		(void)radix_sort(S2, m, K.ref_bits + BIN_BITS, d_hist.p);
		const uint64_t *const key2 = S2.key[S2.in];
		const uint32_t *const val2 = S2.val[S2.in];
		// in the key array the second sort left free, as words: 2 m + 1 of them in an array of 2 n + 4
		const ChunkMarks C{(uint32_t *)S2.key[1 - S2.in], (uint32_t *)S2.key[1 - S2.in] + m};
		hipLaunchKernelGGL(chunk_flag_kernel, dim3(grid_for(m)), dim3(NT), 0, nullptr, key2, val2, m, C.flag);
		scan_launch<uint32_t, uint32_t>(C.flag, m, C.index, d_sums.p);
		HIP_TRY(hipGetLastError());
		uint32_t n_chunks = 0;
		HIP_TRY(hipMemcpy(&n_chunks, C.index + m, 4, hipMemcpyDeviceToHost));
		if (n_chunks > m) return URMAPX_E_NODEVICE;
		if ((rc = d_chunks.alloc(n_chunks))) return rc;
		hipLaunchKernelGGL(chunk_write_kernel, dim3(grid_for(m)), dim3(NT), 0, nullptr, key2, val2, C.flag, C.index, d_dst.p, m, n_chunks, d_chunks.p);
		HIP_TRY(hipGetLastError());
		X.chunks.resize(n_chunks);
		HIP_TRY(hipMemcpy(X.chunks.data(), d_chunks.p, (size_t)n_chunks * sizeof(Chunk), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(X.lin.data(), d_lin.p, n_win * 8, hipMemcpyDeviceToHost));
		return URMAPX_OK;
	}

	// markdup: bit 0x400 of the resident records, before the first of them is copied into order.  On the external road what it reads of
	// the records was taken as they passed (keys_of in the first pass) and the decisions go to d_action, for place_kernel
	int mark_duplicates() {
		if (!md) return URMAPX_OK;
		Span span(md->markdup_s);
		int rc;
		if (!ext && ((rc = W.begin(n)) || (rc = markdup_chunk(W, d_rec.p, 0, d_off.p, 0, n, n, nullptr)))) return rc;
		// What the marking sorts and scores in is used up by now: both key arrays (the index stage's last reader was chunk_write_kernel),
		// the lengths, the second sort's numbers in d_val[2], the ends (lin_kernel, bin_key_kernel).  by_coor.val, d_dst, d_off, d_rec are not
		const MarkdupArrays A{d_rec.p, d_off.p, n, n_ref, {by_coor.key, spare.key}, {lengths, d_val[2].p}, d_end.p, d_hist.p, d_sums.p, ext ? d_action.p : nullptr};
		return markdup_device(A, W, md);
	}

	// What is taken beside the sort, in core: one by-product after the other, each with its launches over the records as they came,
	// now that every bit 0x400 is what the file will hold.  (On the external road the decisions wait in d_action until the records pass
	// again: the first placing pass counts, in partitions)
	int beside_in_core() {
		if (ext) return URMAPX_OK;
		for (Beside *B : beside) {
			Span span(*B->count_s);
			if (const int rc = B->count(d_rec.p, 0, d_off.p, 0, n, nullptr, nullptr)) return rc;
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(nullptr));
		}
		return URMAPX_OK;
	}

	// the sorted stream, a slice at a time: into order, deflate, copy back
	int sorted_stream() {
		slice_bytes = (size_t)slice_members() * MEMBER;
		const size_t slice_cap = slice_bytes < n_bytes ? slice_bytes : n_bytes;
		z_cap = urmapx_bgzf_bound(slice_cap);
		int rc;
		if ((!ext && (rc = d_slice.alloc(slice_cap + 16))) || (rc = d_z.alloc(z_cap + 16)) || (rc = d_used.alloc(1))) return rc;
		urmapx_bgzf *made = nullptr;
		if ((rc = urmapx_bgzf_create(device, nullptr, &made))) return rc;
		Z.reset(made);
		host_cap = urmapx_bgzf_bound(n_bytes);
		z.reset((uint8_t *)malloc(host_cap ? host_cap : 1));
		rc = !z ? URMAPX_E_NOMEM : ext ? partitions() : slices();
		Z.reset();  // (the compressor's device memory goes before the by-products' finish() ask for their own)
		return rc;
	}
	// a slice that lies on the device: deflate, copy back
	int members(const uint8_t *d_in, size_t bytes) {
		uint64_t used = 0;
		{
			Span span(out->deflate_s);
			if (const int r = urmapx_bgzf_compress_device(device, d_in, bytes, d_z.p, z_cap, d_used.p, 0, Z.get())) return r;
			HIP_TRY(hipMemcpy(&used, d_used.p, 8, hipMemcpyDeviceToHost));
		}
		if (used > z_cap || z_bytes + used > host_cap) return URMAPX_E_NODEVICE;
		Span span(out->copy_s);
		if (used) HIP_TRY(hipMemcpy(z.get() + z_bytes, d_z.p, (size_t)used, hipMemcpyDeviceToHost));
		z_bytes += (size_t)used;
		++out->slices;
		return URMAPX_OK;
	}
	int slices() {
		for (uint64_t s0 = 0; s0 < n_bytes; s0 += slice_bytes) {
			const uint64_t s1 = s0 + slice_bytes < n_bytes ? s0 + slice_bytes : n_bytes;
			{
				Span span(out->gather_s);
				hipLaunchKernelGGL(slice_range_kernel, dim3(1), dim3(1), 0, nullptr, d_dst.p, n, s0, s1, d_range.p);
				hipLaunchKernelGGL(gather_kernel, dim3(4096), dim3(NT), 0, nullptr, d_rec.p, d_off.p, by_coor.val, d_dst.p, d_range.p, s0, s1, d_slice.p);
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipStreamSynchronize(nullptr));
			}
			if (const int r = members(d_slice.p, (size_t)(s1 - s0))) return r;
		}
		return URMAPX_OK;
	}
	// The external road: where every record of the input goes, then partition after partition: the input passes through the staging
	// buffers once more, place_kernel fills the partition, and its slices -- partitions end on slice ends, so they are the in-core
	// road's slices -- are deflated and copied back
	int partitions() {
		place = spare.key;  // (both key arrays are used up: the index stage, then the marking)
		if (n) hipLaunchKernelGGL(place_fill_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, by_coor.val, d_dst.p, n, place);
		HIP_TRY(hipGetLastError());
		const uint8_t *const action = md ? d_action.p : nullptr;
		for (uint64_t p0 = 0; p0 < n_bytes; p0 += P.partition_bytes) {
			const uint64_t p1 = p0 + P.partition_bytes < n_bytes ? p0 + P.partition_bytes : n_bytes;
			// (every record crosses the device in each of these passes: the by-products are taken in the first one only)
			int r = pass(false, [&](const uint8_t *at, uint64_t base, uint32_t i0, uint32_t i1, hipStream_t s) -> int {
				hipLaunchKernelGGL(place_kernel, dim3(grid_for(i1 - i0)), dim3(NT), 0, s, at, base, d_off.p, i0, i1, place, action, p0, p1, d_part.p);
				if (p0 == 0)
					for (Beside *B : beside)
						if (const int e = B->count(at, base, d_off.p, i0, i1, action, s)) return e;
				return URMAPX_OK;
			});
			if (r) return r;
			for (uint64_t s0 = p0; s0 < p1; s0 += slice_bytes) {
				const uint64_t s1 = s0 + slice_bytes < p1 ? s0 + slice_bytes : p1;
				if ((r = members(d_part.p + (s0 - p0), (size_t)(s1 - s0)))) return r;
			}
		}
		return URMAPX_OK;
	}

	// the by-products' results, then the sort's: the members trimmed to their size and handed to finish_result, which owns them from there
	int finish() {
		for (Beside *B : beside)
			if (const int rc = B->finish()) return rc;
		if (uint8_t *fit = (uint8_t *)realloc(z.get(), z_bytes ? z_bytes : 1)) {
			(void)z.release();
			z.reset(fit);
		}
		Span span(out->index_s);
		return finish_result(out, z.release(), z_bytes, n_bytes, in_front, X, n_ref);
	}
};

}  // namespace

extern "C" {

uint64_t urmapx_bam_sort_device_bytes(size_t n_bytes, uint64_t n_records) {
	const size_t slice = (size_t)slice_members() * MEMBER;
	return (uint64_t)n_bytes + SORT_PER_RECORD * n_records + slice_scratch_bytes(slice < n_bytes ? slice : n_bytes) + SORT_SLACK;
}

uint64_t urmapx_bam_sort_markdup_device_bytes(size_t n_bytes, uint64_t n_records) {
	return urmapx_bam_sort_device_bytes(n_bytes, n_records) + MARKDUP_PER_RECORD * n_records + 4096u;
}

static int sort_entry(int device, const uint64_t *budget, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                      size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out, const std::vector<Beside *> &beside = {}) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	if (md) memset(md, 0, sizeof *md);
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	int rc;
	try {
		t_alloc_s = 0;
		uint64_t have = budget ? *budget : 0;
		if (budget && have == 0) {  // what is free, less the headroom
			size_t free_b = 0, total_b = 0;
			HIP_TRY(hipSetDevice(device));
			HIP_TRY(hipMemGetInfo(&free_b, &total_b));
			have = free_b > URMAPX_SORT_HEADROOM ? (uint64_t)free_b - URMAPX_SORT_HEADROOM : 1u;
		}
		rc = DeviceSort{device, budget ? &have : nullptr, (const uint8_t *)records, n_bytes, n_ref, bytes_in_front, starts, n_starts, md, beside, out}.run();
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	out->alloc_s = t_alloc_s;  // (the arrays are freed by now)
	if (rc) urmapx_bam_sort_free(out);
	if (rc)
		for (Beside *B : beside) B->free_result();
	return rc;
}

int urmapx_bam_sort(int device, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                    size_t n_starts, urmapx_bam_sort_result *out) {
	return sort_entry(device, nullptr, records, n_bytes, n_ref, bytes_in_front, starts, n_starts, nullptr, out);
}

int urmapx_bam_sort_markdup(int device, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                            size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out) {
	if (!md) return URMAPX_E_ARG;
	return sort_entry(device, nullptr, records, n_bytes, n_ref, bytes_in_front, starts, n_starts, md, out);
}

int urmapx_bam_sort_external(int device, uint64_t budget_bytes, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front,
                             const uint64_t *starts, size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out) {
	return sort_entry(device, &budget_bytes, records, n_bytes, n_ref, bytes_in_front, starts, n_starts, md, out);
}

int urmapx_bam_sort_with(int device, uint64_t budget_bytes, const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front,
                         const uint64_t *starts, size_t n_starts, const urmapx_bam_sort_extras *extras, urmapx_bam_sort_result *out) {
	const urmapx_bam_sort_extras none{};
	const urmapx_bam_sort_extras &E = extras ? *extras : none;
	if (!E.depth && !E.stats && !E.pileup) return sort_entry(device, &budget_bytes, records, n_bytes, n_ref, bytes_in_front, starts, n_starts, E.md, out);
	if (E.depth) memset(E.depth, 0, sizeof *E.depth);
	if (E.stats) memset(E.stats, 0, sizeof *E.stats);
	if (E.pileup) memset(E.pileup, 0, sizeof *E.pileup);
	uint64_t entries = 0, columns = 0;
	if (const int rc = urx::depth::check_refs(n_ref, E.names, E.lens, &entries)) return rc;
	columns = entries - n_ref;
	urx::pileup::Rule R;
	const uint8_t *const *seqs = E.seqs;
	const uint8_t *d_store = nullptr;
	// the bases: the caller's, or the index's -- in place where its store is resident on this device, else fetched once to the host
	std::vector<uint8_t> fetched;
	std::vector<const uint8_t *> fetched_at;
	std::vector<uint64_t> store_at;
	if (E.pileup) {
		if (const int rc = urx::pileup::rule_of(E.popts, &R)) return rc;
		if (!E.seqs) {
			if (!E.index || urmapx_index_seq_count(E.index) != n_ref) return URMAPX_E_ARG;
			const urx::IndexStore S = urx::index_store(E.index);
			if (S.d_seq && S.device == device) {
				store_at.resize((size_t)n_ref + 1, 0);
				for (uint32_t r = 0; r < n_ref; ++r) {
					store_at[r] = urmapx_index_seq_offset(E.index, r);
					if (urmapx_index_seq_length(E.index, r) != E.lens[r] || store_at[r] + E.lens[r] > S.seq_data_size) return URMAPX_E_ARG;
				}
				d_store = S.d_seq;
			} else {
				try {
					if (const int rc = urx::pileup::index_sequences(E.index, n_ref, E.lens, fetched, fetched_at)) return rc;
				} catch (const std::bad_alloc &) {
					return URMAPX_E_NOMEM;
				}
				seqs = fetched_at.data();
			}
		}
		if (seqs)
			if (const int rc = urx::pileup::check_input(n_ref, E.names, E.lens, seqs, &columns)) return rc;
	}
	// what is taken beside the sort: the one place that names them.  Their arrays go when this scope ends, and count in alloc_s
	int rc;
	{
		std::optional<urx::depth::DepthBeside> dep;
		std::optional<urx::stats::StatsBeside> sta;
		std::optional<urx::pileup::PileupBeside> pil;
		std::vector<Beside *> beside;
		if (E.depth) beside.push_back(&dep.emplace(n_ref, E.names, E.lens, entries, E.dopts ? E.dopts->min_mapq : 0u, E.depth));
		if (E.stats) beside.push_back(&sta.emplace(n_ref, E.names, E.lens, E.stats_command, E.stats));
		if (E.pileup) beside.push_back(&pil.emplace(n_ref, R, E.names, E.lens, columns, seqs, d_store, d_store ? store_at.data() : nullptr, E.pileup_command, E.pileup));
		rc = sort_entry(device, &budget_bytes, records, n_bytes, n_ref, bytes_in_front, starts, n_starts, E.md, out, beside);
	}
	if (out) out->alloc_s = t_alloc_s;
	return rc;
}

}  // extern "C"
