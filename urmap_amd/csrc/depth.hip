// depth.hip -- per-base depth of BAM records on the device (urmapx_bam_depth, and the depth step of urmapx_bam_sort_with; the rule is
// in include/urmapx.h "Depth", the sizes and the memory sum in depth.h, the host version in depth_host.cpp).
//
// The counters are one uint32 array in which reference r owns l_ref + 1 entries from base[r] on; all their arithmetic is modulo 2^32,
// which is exact: every depth lies below 2^31.
//
//   depth_count_kernel   one THREAD per record: the eligibility test, then the CIGAR walk with +1 at the first covered column of an
//                        M, = or X op and -1 behind its last (atomicAdd; an end beyond the reference lands in the extra entry).  A
//                        lane walks at most LANE_OPS ops alone; a record with more is taken by the whole wavefront afterwards, 64 ops
//                        at a time: every lane loads one op, a shuffle scan of the reference-consuming lengths gives each its cursor.
//                        reads and mapq_sum: the lanes of a wavefront that share a reference add up (ballot, shuffle reduction) and
//                        one of them does the atomic
//   scan_reduce / block_scan / scan_apply   the inclusive scan in place, reduce-then-scan: workgroup b owns a contiguous range of
//                        whole tiles, sums it, one workgroup scans the SCAN_BLOCKS sums, then every workgroup walks its range tile by
//                        tile with a running carry (eight counters a thread, a shuffle scan per wavefront, the four wavefronts
//                        through LDS).  Indices are 64 bits wide
//   runs_count / runs_write   a segment of SEGMENT counters at a time: a thread looks at eight neighbouring counters (one binary search
//                        for the reference of the first, then it walks), flags a column that begins a reference or differs from the
//                        column in front (never the extra entry), and the workgroup counts its flags; the counts are scanned and the
//                        second kernel, which finds the same flags again, writes the flagged places into the run list.  The first
//                        kernel also sums covered and bases: per wavefront, the four through LDS, one atomic per reference touched
//   line_len / block_scan / line_write   a slice of the run list at a time: the length of every line, their starts, the bytes.  A run
//                        ends where the next one starts if that is on the same reference, else at the reference's end
#include "depth_dev.h"
#include "block_scan_dev.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace urx::bamsort;
using namespace urx::depth;
using urx::devscan::block_scan_kernel;
using urx::devscan::BS_NT;

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr uint32_t DNT = urx::depth::NT;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t from) { return (uint32_t)__shfl((int)v, (int)from, 64); }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t from) { return (uint64_t)shfl32((uint32_t)(v >> 32), from) << 32 | shfl32((uint32_t)v, from); }
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t by) {
	return (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), by, 64) << 32 | (uint32_t)__shfl_up((int)(uint32_t)v, by, 64);
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
	for (int s = 32; s; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
	return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
	for (int s = 32; s; s >>= 1) v += (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64);
	return v;
}
// the inclusive sums of v over the lanes of a wavefront
__device__ __forceinline__ uint32_t wave_scan32(uint32_t v) {
	for (uint32_t by = 1; by < 64u; by <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)v, by, 64);
		if (lane_id() >= by) v += t;
	}
	return v;
}

// the reference that owns counter g: the largest r below n_ref with base[r] <= g (g < base[n_ref], n_ref >= 1)
__device__ __forceinline__ uint32_t ref_of(const uint64_t *base, uint32_t n_ref, uint64_t g) {
	uint32_t lo = 0, hi = n_ref;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (base[mid] <= g) lo = mid; else hi = mid;
	}
	return lo;
}

// ---- counting ----
// columns [c, c + len) of a reference of l_ref columns whose counters begin at diff + b
__device__ __forceinline__ void cover(uint32_t *diff, uint64_t b, uint64_t l_ref, uint64_t c, uint64_t len) {
	if (len == 0 || c >= l_ref) return;
	const uint64_t e = c + len < l_ref ? c + len : l_ref;
	atomicAdd(diff + (b + c), 1u);
	atomicAdd(diff + (b + e), 0xFFFFFFFFu);
}
__device__ __forceinline__ bool covers(uint32_t op) { return op == 0u || op == 7u || op == 8u; }

__global__ __launch_bounds__(DNT) void depth_count_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action,
                                                          uint32_t min_mapq, uint32_t n_ref, const uint64_t *ref_base, uint32_t *diff, unsigned long long *stat) {
	const uint32_t n = i1 - i0, lane = lane_id();
	for (uint64_t k0 = (uint64_t)blockIdx.x * DNT; k0 < n; k0 += (uint64_t)gridDim.x * DNT) {  // (the same trips for every lane of a workgroup)
		const uint64_t k = k0 + threadIdx.x;
		bool eligible = false;
		uint32_t ref = 0, mapq = 0, n_cigar = 0;
		uint64_t pos = 0;
		const uint8_t *cig = rec;
		if (k < n) {
			const uint64_t i = i0 + k;
			const uint8_t *r = rec + (off[i] - base);
			const uint64_t len = off[i + 1] - off[i];
			const uint32_t p = load_u32(r + 8), w3 = load_u32(r + 12), w4 = load_u32(r + 16);
			ref = load_u32(r + 4);
			uint32_t flag = w4 >> 16;
			if (action) {
				const uint8_t a = action[i];
				if (a == MD_SET) flag |= 0x400u;
				else if (a == MD_CLEAR) flag &= ~0x400u;
			}
			mapq = w3 >> 8 & 0xFFu;
			const uint32_t l_name = w3 & 0xFFu;
			n_cigar = w4 & 0xFFFFu;
			eligible = ref < n_ref && !(p >> 31) && !(flag & 0x704u) && mapq >= min_mapq;
			if ((uint64_t)CORE + l_name + 4ull * n_cigar > len) n_cigar = 0;  // (scan_records has refused such a record)
			pos = p;
			cig = r + CORE + l_name;
		}
		// reads and mapq_sum: the lanes of one reference at a time
		for (unsigned long long todo = __ballot(eligible); todo;) {
			const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u, r0 = shfl32(ref, leader);
			const bool mine = eligible && ref == r0;
			const unsigned long long m = __ballot(mine);
			const uint32_t q = wave_sum32(mine ? mapq : 0u);
			if (lane == leader) {
				atomicAdd(stat + 4ull * r0, (unsigned long long)__popcll(m));
				atomicAdd(stat + 4ull * r0 + 3u, (unsigned long long)q);
			}
			todo &= ~m;
		}
		// the short CIGARs: a lane each
		const bool shared = eligible && n_cigar > LANE_OPS;
		if (eligible && !shared) {
			const uint64_t b = ref_base[ref], l_ref = ref_base[ref + 1] - b - 1u;
			uint64_t c = pos;
			for (uint32_t o = 0; o < n_cigar; ++o) {
				const uint32_t w = load_u32(cig + 4u * o), op = w & 15u;
				if (covers(op)) cover(diff, b, l_ref, c, w >> 4);
				if (consumes_ref(op)) c += w >> 4;
			}
		}
		// the long ones: the wavefront takes them one after the other, 64 ops at a time
		for (unsigned long long todo = __ballot(shared); todo; todo &= todo - 1u) {
			const uint32_t src = (uint32_t)__ffsll((long long)todo) - 1u;
			const uint32_t r0 = shfl32(ref, src), ops = shfl32(n_cigar, src);
			const uint8_t *cg = (const uint8_t *)shfl64((uint64_t)cig, src);
			const uint64_t b = ref_base[r0], l_ref = ref_base[r0 + 1] - b - 1u;
			uint64_t at = shfl64(pos, src);  // the cursor in front of op o0
			for (uint32_t o0 = 0; o0 < ops; o0 += 64u) {
				const uint32_t o = o0 + lane;
				const uint32_t w = o < ops ? load_u32(cg + 4ull * o) : 0u, op = w & 15u;
				const uint64_t adv = o < ops && consumes_ref(op) ? (uint64_t)(w >> 4) : 0u;
				uint64_t inc = adv;
				for (uint32_t by = 1; by < 64u; by <<= 1) {
					const uint64_t t = shfl_up64(inc, by);
					if (lane >= by) inc += t;
				}
				if (o < ops && covers(op)) cover(diff, b, l_ref, at + inc - adv, w >> 4);
				at += shfl64(inc, 63);
			}
		}
	}
}

// ---- the scan (block_scan_kernel: block_scan_dev.h) ----
// eight neighbouring counters from g on, those from g1 on as 0 (g is a multiple of eight: the array comes from hipMalloc)
__device__ __forceinline__ void load8(const uint32_t *d, uint64_t g, uint64_t g1, uint32_t (&v)[SCAN_ITEMS]) {
	if (g + SCAN_ITEMS <= g1) {
		const uint4 a = *(const uint4 *)(d + g), b = *(const uint4 *)(d + g + 4);
		v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
	} else {
#pragma unroll
		for (uint32_t k = 0; k < SCAN_ITEMS; ++k) v[k] = g + k < g1 ? d[g + k] : 0u;
	}
}

// workgroup b owns counters [b * per_block, min(n, (b + 1) * per_block)); per_block is a multiple of SCAN_TILE
__global__ __launch_bounds__(DNT) void scan_reduce_kernel(const uint32_t *d, uint64_t n, uint64_t per_block, uint32_t *sums) {
	__shared__ uint32_t s_w[DNT / 64];
	const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
	uint32_t s = 0;
	for (uint64_t g = lo + (uint64_t)threadIdx.x * SCAN_ITEMS; g < hi; g += SCAN_TILE) {
		uint32_t v[SCAN_ITEMS];
		load8(d, g, hi, v);
#pragma unroll
		for (uint32_t k = 0; k < SCAN_ITEMS; ++k) s += v[k];
	}
	s = wave_sum32(s);
	if (lane_id() == 0) s_w[threadIdx.x >> 6] = s;
	__syncthreads();
	if (threadIdx.x == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// sums[b]: what lies in front of workgroup b's range
__global__ __launch_bounds__(DNT) void scan_apply_kernel(uint32_t *d, uint64_t n, uint64_t per_block, const uint32_t *sums) {
	__shared__ uint32_t s_w[DNT / 64];
	const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = lo + per_block < n ? lo + per_block : n;
	const uint32_t wave = threadIdx.x >> 6;
	uint32_t carry = sums[blockIdx.x];
	for (uint64_t tile = lo; tile < hi; tile += SCAN_TILE) {  // (the same trips for every thread)
		const uint64_t g = tile + (uint64_t)threadIdx.x * SCAN_ITEMS;
		uint32_t v[SCAN_ITEMS];
		load8(d, g < hi ? g : hi, hi, v);
#pragma unroll
		for (uint32_t k = 1; k < SCAN_ITEMS; ++k) v[k] += v[k - 1];
		const uint32_t mine = v[SCAN_ITEMS - 1], inc = wave_scan32(mine);
		if (lane_id() == 63u) s_w[wave] = inc;
		__syncthreads();
		uint32_t front = carry + inc - mine, total = 0;
#pragma unroll
		for (uint32_t w = 0; w < DNT / 64; ++w) {
			if (w < wave) front += s_w[w];
			total += s_w[w];
		}
		if (g + SCAN_ITEMS <= hi) {
			*(uint4 *)(d + g) = make_uint4(v[0] + front, v[1] + front, v[2] + front, v[3] + front);
			*(uint4 *)(d + g + 4) = make_uint4(v[4] + front, v[5] + front, v[6] + front, v[7] + front);
		} else {
#pragma unroll
			for (uint32_t k = 0; k < SCAN_ITEMS; ++k)
				if (g + k < hi) d[g + k] = v[k] + front;
		}
		carry += total;
		__syncthreads();
	}
}

// ---- the runs ----
// Counters [g0, g1) (at most eight, g0 a multiple of eight) of the scanned array: bit k of the result says that g0 + k begins a run.
// STATS: covered and bases of the reference the thread ends on go to cov and sum, those of references it leaves straight to stat.
// r: that reference.  Nothing at all for g0 >= g1
template <bool STATS>
__device__ __forceinline__ uint32_t run_flags(const uint32_t *d, const uint64_t *base, uint32_t n_ref, uint64_t g0, uint64_t g1, uint32_t &r, uint32_t &cov,
                                              uint64_t &sum, unsigned long long *stat) {
	if (g0 >= g1) return 0u;
	uint32_t v[SCAN_ITEMS];
	load8(d, g0, g1, v);
	r = ref_of(base, n_ref, g0);
	uint64_t first = base[r], next = base[r + 1];
	uint32_t prev = g0 ? d[g0 - 1] : 0u, mask = 0;
#pragma unroll
	for (uint32_t k = 0; k < SCAN_ITEMS; ++k) {
		const uint64_t g = g0 + k;
		if (g < g1) {
			while (g >= next) {  // (g < g1 <= base[n_ref]: r stays below n_ref)
				if (STATS && (cov | sum)) {
					atomicAdd(stat + 4ull * r + 1u, (unsigned long long)cov);
					atomicAdd(stat + 4ull * r + 2u, (unsigned long long)sum);
				}
				cov = 0; sum = 0;
				++r;
				first = next;
				next = base[r + 1];
			}
			if (g != next - 1u) {  // (the last entry of a reference is no column)
				if (g == first || v[k] != prev) mask |= 1u << k;
				if (STATS && v[k]) { ++cov; sum += v[k]; }
			}
			prev = v[k];
		}
	}
	return mask;
}

// the segment [s0, s1): workgroup b looks at RUN_TILE counters from s0 + b * RUN_TILE on
__global__ __launch_bounds__(DNT) void runs_count_kernel(const uint32_t *d, const uint64_t *base, uint32_t n_ref, uint64_t s0, uint64_t s1, uint32_t *bcount,
                                                         unsigned long long *stat) {
	__shared__ uint32_t s_cnt[DNT / 64], s_ref[DNT / 64], s_cov[DNT / 64];
	__shared__ uint64_t s_sum[DNT / 64];
	const uint64_t g0 = s0 + (uint64_t)blockIdx.x * RUN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS, g1 = g0 + SCAN_ITEMS < s1 ? g0 + SCAN_ITEMS : s1;
	const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
	uint32_t r = 0xFFFFFFFFu, cov = 0;
	uint64_t sum = 0;
	const uint32_t mask = run_flags<true>(d, base, n_ref, g0, g1, r, cov, sum, stat);
	const uint32_t cnt = wave_sum32((uint32_t)__popc(mask));
	// covered and bases: a wavefront whose lanes ended on one reference adds up; in any other every lane adds its own
	const bool active = g0 < g1;
	const uint32_t r_front = shfl32(r, 0);  // (the lanes with counters are the first ones of a wavefront)
	const bool uniform = __all(!active || r == r_front);
	if (!uniform && active && (cov | sum)) {
		atomicAdd(stat + 4ull * r + 1u, (unsigned long long)cov);
		atomicAdd(stat + 4ull * r + 2u, (unsigned long long)sum);
	}
	const uint32_t w_cov = wave_sum32(uniform ? cov : 0u);
	const uint64_t w_sum = wave_sum64(uniform ? sum : 0u);
	if (lane == 0) {
		s_cnt[wave] = cnt;
		s_ref[wave] = uniform ? r_front : 0xFFFFFFFFu;
		s_cov[wave] = w_cov;
		s_sum[wave] = w_sum;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		bcount[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
		for (uint32_t w = 0; w < DNT / 64;) {  // one atomic per reference the workgroup touched (neighbouring wavefronts share it)
			const uint32_t rr = s_ref[w];
			uint32_t c = 0;
			uint64_t s = 0;
			uint32_t x = w;
			for (; x < DNT / 64 && s_ref[x] == rr; ++x) { c += s_cov[x]; s += s_sum[x]; }
			if (rr != 0xFFFFFFFFu && (c | s)) {
				atomicAdd(stat + 4ull * rr + 1u, (unsigned long long)c);
				atomicAdd(stat + 4ull * rr + 2u, (unsigned long long)s);
			}
			w = x;
		}
	}
}
// boff: the scanned counts; the flagged places go to list[at0 + boff[b] ...] in ascending order
__global__ __launch_bounds__(DNT) void runs_write_kernel(const uint32_t *d, const uint64_t *base, uint32_t n_ref, uint64_t s0, uint64_t s1, const uint32_t *boff,
                                                         uint32_t at0, uint64_t *list) {
	__shared__ uint32_t s_w[DNT / 64];
	const uint64_t g0 = s0 + (uint64_t)blockIdx.x * RUN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS, g1 = g0 + SCAN_ITEMS < s1 ? g0 + SCAN_ITEMS : s1;
	const uint32_t wave = threadIdx.x >> 6;
	uint32_t r = 0, cov = 0;
	uint64_t sum = 0;
	const uint32_t mask = run_flags<false>(d, base, n_ref, g0, g1, r, cov, sum, nullptr);
	const uint32_t mine = (uint32_t)__popc(mask), inc = wave_scan32(mine);
	if (lane_id() == 63u) s_w[wave] = inc;
	__syncthreads();
	uint64_t at = (uint64_t)at0 + boff[blockIdx.x] + inc - mine;
	for (uint32_t w = 0; w < wave; ++w) at += s_w[w];
	for (uint32_t m = mask; m; m &= m - 1u) list[at++] = g0 + (uint32_t)(__ffs((int)m) - 1);
}

// ---- the text ----
struct Run {
	uint32_t ref, depth;
	uint64_t beg, end;
};
// run j of the list: it ends where the next one starts if that lies on the same reference (list[j + 1]: the next start or the end of all)
__device__ __forceinline__ Run run_of(const uint64_t *list, uint32_t j, const uint32_t *d, const uint64_t *base, uint32_t n_ref) {
	const uint64_t g = list[j], next = list[j + 1];
	Run R;
	R.ref = ref_of(base, n_ref, g);
	const uint64_t first = base[R.ref], l_ref = base[R.ref + 1] - first - 1u;
	R.beg = g - first;
	R.end = next < first + l_ref ? next - first : l_ref;
	R.depth = d[g];
	return R;
}
__device__ __forceinline__ uint32_t digits_of(uint64_t v) {
	uint32_t n = 1;
	while (v >= 10u) { v /= 10u; ++n; }
	return n;
}
// v in decimal, its last digit at p[-1]; -> where the first one went
__device__ __forceinline__ uint8_t *put_backwards(uint8_t *p, uint64_t v) {
	do { *--p = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
	return p;
}
__global__ __launch_bounds__(DNT) void line_len_kernel(const uint64_t *list, uint32_t j0, uint32_t j1, const uint32_t *d, const uint64_t *base, uint32_t n_ref,
                                                       const uint8_t *names, uint32_t *len) {
	for (uint32_t j = j0 + blockIdx.x * DNT + threadIdx.x; j < j1; j += gridDim.x * DNT) {
		const Run R = run_of(list, j, d, base, n_ref);
		len[j - j0] = names[(uint64_t)R.ref * NAME_SLOT] + 4u + digits_of(R.beg) + digits_of(R.end) + digits_of(R.depth);
	}
}
__global__ __launch_bounds__(DNT) void line_write_kernel(const uint64_t *list, uint32_t j0, uint32_t j1, const uint32_t *d, const uint64_t *base, uint32_t n_ref,
                                                         const uint8_t *names, const uint64_t *at, uint8_t *text) {
	for (uint32_t j = j0 + blockIdx.x * DNT + threadIdx.x; j < j1; j += gridDim.x * DNT) {
		const Run R = run_of(list, j, d, base, n_ref);
		const uint8_t *nm = names + (uint64_t)R.ref * NAME_SLOT;
		uint8_t *p = text + at[j - j0];
		for (uint32_t k = 0; k < nm[0]; ++k) *p++ = nm[1 + k];
		uint8_t *e = text + at[j - j0 + 1];  // the line is written from its end: every number's length is known by where the next begins
		*--e = '\n';
		e = put_backwards(e, R.depth);
		*--e = '\t';
		e = put_backwards(e, R.end);
		*--e = '\t';
		e = put_backwards(e, R.beg);
		*--e = '\t';
	}
}

// the text as it grows on the host (malloc: the result owns it in the end)
struct HostText {
	char *p = nullptr;
	size_t used = 0, cap = 0;
	int append(const void *from, size_t n) {
		if (used + n > cap) {
			size_t want = cap ? cap * 2 : (size_t)1 << 20;
			while (want < used + n) want *= 2;
			char *q = (char *)realloc(p, want);
			if (!q) return URMAPX_E_NOMEM;
			p = q; cap = want;
		}
		if (n) memcpy(p + used, from, n);
		used += n;
		return URMAPX_OK;
	}
	~HostText() { free(p); }
};

inline uint32_t grid_of(uint64_t n, uint32_t most = 4096) {
	const uint64_t g = (n + DNT - 1) / DNT;
	return (uint32_t)(g < 1 ? 1 : g > most ? most : g);
}

}  // namespace

namespace urx {
namespace depth {

int DepthOwn::begin(uint32_t n_ref_, const char *const *names_, const uint32_t *lens, uint64_t entries_) {
	n_ref = n_ref_;
	entries = entries_;
	slice_runs = text_runs();
	const uint64_t seg = entries < SEGMENT ? entries : SEGMENT;
	int rc;
	if ((rc = diff.alloc((size_t)entries)) || (rc = base.alloc((size_t)n_ref + 1)) || (rc = names.alloc((size_t)NAME_SLOT * n_ref)) ||
	    (rc = stat.alloc((size_t)4 * n_ref)) || (rc = list.alloc((size_t)seg + 2)) || (rc = bcount.alloc(RUN_BLOCKS + 1)) || (rc = ssum.alloc(SCAN_BLOCKS + 1)))
		return rc;
	for (int b = 0; b < 2; ++b)
		if ((rc = text[b].alloc((size_t)slice_runs * LINE_MOST)) || (rc = llen[b].alloc(slice_runs)) || (rc = loff[b].alloc((size_t)slice_runs + 1))) return rc;
	std::vector<uint64_t> h_base((size_t)n_ref + 1, 0);
	std::vector<uint8_t> h_names((size_t)NAME_SLOT * n_ref, 0);
	for (uint32_t r = 0; r < n_ref; ++r) {
		h_base[r + 1] = h_base[r] + lens[r] + 1u;
		const size_t l = strlen(names_[r]);  // (1 .. MAX_NAME: check_refs)
		h_names[(size_t)NAME_SLOT * r] = (uint8_t)l;
		memcpy(&h_names[(size_t)NAME_SLOT * r + 1], names_[r], l);
	}
	if (h_base[n_ref] != entries) return URMAPX_E_ARG;
	HIP_TRY(hipMemcpy(base.p, h_base.data(), h_base.size() * 8, hipMemcpyHostToDevice));
	if (n_ref) HIP_TRY(hipMemcpy(names.p, h_names.data(), h_names.size(), hipMemcpyHostToDevice));
	HIP_TRY(hipMemset(diff.p, 0, (size_t)(entries ? entries : 1) * 4));
	HIP_TRY(hipMemset(stat.p, 0, (size_t)(n_ref ? 4 * (size_t)n_ref : 1) * 8));
	return URMAPX_OK;
}

int depth_count(const DepthOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, uint32_t min_mapq,
                hipStream_t stream) {
	if (i1 <= i0 || W.n_ref == 0) return URMAPX_OK;
	hipLaunchKernelGGL(depth_count_kernel, dim3(grid_of(i1 - i0, COUNT_BLOCKS)), dim3(DNT), 0, stream, rec, base, off, i0, i1, action, min_mapq, W.n_ref, (const uint64_t *)W.base.p,
	                   W.diff.p, W.stat.p);
	return URMAPX_OK;
}

int depth_finish(DepthOwn &W, urmapx_depth_result *out) {
	const uint64_t E = W.entries;
	const uint32_t n_ref = W.n_ref;
	out->n_ref = n_ref;
	out->refs = (urmapx_depth_summary *)calloc(n_ref ? n_ref : 1, sizeof(urmapx_depth_summary));
	if (!out->refs) return URMAPX_E_NOMEM;
	HIP_TRY(hipDeviceSynchronize());

	// the differences become depths
	auto t = Clock::now();
	if (E) {
		const uint64_t tiles = (E + SCAN_TILE - 1) / SCAN_TILE, blocks = tiles < SCAN_BLOCKS ? tiles : SCAN_BLOCKS;
		const uint64_t per_block = (tiles + blocks - 1) / blocks * SCAN_TILE;
		hipLaunchKernelGGL(scan_reduce_kernel, dim3((uint32_t)blocks), dim3(DNT), 0, nullptr, (const uint32_t *)W.diff.p, E, per_block, W.ssum.p);
		hipLaunchKernelGGL((block_scan_kernel<uint32_t>), dim3(1), dim3(BS_NT), 0, nullptr, (const uint32_t *)W.ssum.p, W.ssum.p, (uint32_t)blocks, 0);
		hipLaunchKernelGGL(scan_apply_kernel, dim3((uint32_t)blocks), dim3(DNT), 0, nullptr, W.diff.p, E, per_block, (const uint32_t *)W.ssum.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(nullptr));
	}
	out->scan_s = since(t);

	// Segment after segment: its run starts behind the one carried over (the last run of a segment is written with the next segment: its
	// end is not known before).  The lines of slice k are made on stream k & 1 in text[k & 1] and copied to a page-locked buffer of their
	// own while slice k + 1 is made on the other stream; a buffer's lines are appended to the text when its stream is next waited for
	const uint32_t slice = W.slice_runs;
	Pinned h_text[2], h_total;
	TwoStreams st;
	HostText T;
	int rc;
	if ((rc = h_text[0].alloc((size_t)slice * LINE_MOST)) || (rc = h_text[1].alloc((size_t)slice * LINE_MOST)) || (rc = h_total.alloc(16)) || (rc = st.create()))
		return rc;
	uint64_t pending[2] = {0, 0}, n_slices = 0, carried = 0;
	auto collect = [&](int b) -> int {  // what stream b was copying
		const auto t0 = Clock::now();
		HIP_TRY(hipStreamSynchronize(st.s[b]));
		const int r = T.append(h_text[b].p, (size_t)pending[b]);
		pending[b] = 0;
		out->copy_s += since(t0);
		return r;
	};
	auto drain = [&]() -> int {  // the older slice first
		for (uint64_t k = n_slices >= 2 ? n_slices - 2 : 0; k < n_slices; ++k)
			if (int r = collect((int)(k & 1u))) return r;
		return URMAPX_OK;
	};
	for (uint64_t s0 = 0; s0 < E; s0 += SEGMENT) {
		const uint64_t s1 = s0 + SEGMENT < E ? s0 + SEGMENT : E;
		const bool last = s1 == E;
		t = Clock::now();
		const uint32_t blocks = (uint32_t)((s1 - s0 + RUN_TILE - 1) / RUN_TILE);
		uint32_t found = 0;
		hipLaunchKernelGGL(runs_count_kernel, dim3(blocks), dim3(DNT), 0, nullptr, (const uint32_t *)W.diff.p, (const uint64_t *)W.base.p, n_ref, s0, s1, W.bcount.p,
		                   W.stat.p);
		hipLaunchKernelGGL((block_scan_kernel<uint32_t>), dim3(1), dim3(BS_NT), 0, nullptr, (const uint32_t *)W.bcount.p, W.bcount.p, blocks, 1);
		hipLaunchKernelGGL(runs_write_kernel, dim3(blocks), dim3(DNT), 0, nullptr, (const uint32_t *)W.diff.p, (const uint64_t *)W.base.p, n_ref, s0, s1,
		                   (const uint32_t *)W.bcount.p, (uint32_t)carried, W.list.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(&found, W.bcount.p + blocks, 4, hipMemcpyDeviceToHost));
		if (found > s1 - s0) return URMAPX_E_NODEVICE;
		const uint64_t have = carried + found;  // entries of the list
		if (last) HIP_TRY(hipMemcpy(W.list.p + have, &E, 8, hipMemcpyHostToDevice));
		const uint64_t lines = last ? have : have ? have - 1 : 0;
		out->runs_s += since(t);
		for (uint64_t j0 = 0; j0 < lines; j0 += slice) {
			const uint32_t j1 = (uint32_t)(j0 + slice < lines ? j0 + slice : lines), cnt = j1 - (uint32_t)j0;
			const int b = (int)(n_slices & 1u);
			if ((rc = collect(b))) return rc;
			t = Clock::now();
			hipLaunchKernelGGL(line_len_kernel, dim3(grid_of(cnt)), dim3(DNT), 0, st.s[b], (const uint64_t *)W.list.p, (uint32_t)j0, j1, (const uint32_t *)W.diff.p,
			                   (const uint64_t *)W.base.p, n_ref, (const uint8_t *)W.names.p, W.llen[b].p);
			hipLaunchKernelGGL((block_scan_kernel<uint64_t>), dim3(1), dim3(BS_NT), 0, st.s[b], (const uint32_t *)W.llen[b].p, W.loff[b].p, cnt, 1);
			uint64_t *total = (uint64_t *)h_total.p + b;
			HIP_TRY(hipMemcpyAsync(total, W.loff[b].p + cnt, 8, hipMemcpyDeviceToHost, st.s[b]));
			HIP_TRY(hipStreamSynchronize(st.s[b]));
			if (*total > (uint64_t)cnt * LINE_MOST) return URMAPX_E_NODEVICE;
			hipLaunchKernelGGL(line_write_kernel, dim3(grid_of(cnt)), dim3(DNT), 0, st.s[b], (const uint64_t *)W.list.p, (uint32_t)j0, j1, (const uint32_t *)W.diff.p,
			                   (const uint64_t *)W.base.p, n_ref, (const uint8_t *)W.names.p, (const uint64_t *)W.loff[b].p, W.text[b].p);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(h_text[b].p, W.text[b].p, (size_t)*total, hipMemcpyDeviceToHost, st.s[b]));
			pending[b] = *total;
			++n_slices;
			out->runs += cnt;
			out->format_s += since(t);
		}
		// the list is written again by the next segment: its readers end first, then its last entry moves to the front
		if ((rc = drain())) return rc;
		if (!last && have) {
			if (have > 1) HIP_TRY(hipMemcpy(W.list.p, W.list.p + (have - 1), 8, hipMemcpyDeviceToDevice));
			carried = 1;
		}
	}
	out->text_slices = (uint32_t)n_slices;
	if (n_ref) HIP_TRY(hipMemcpy(out->refs, W.stat.p, (size_t)n_ref * sizeof(urmapx_depth_summary), hipMemcpyDeviceToHost));
	if (char *fit = (char *)realloc(T.p, T.used ? T.used : 1)) T.p = fit;
	out->text = T.p;
	out->text_bytes = T.used;
	T.p = nullptr;
	return URMAPX_OK;
}

uint64_t DepthBeside::resident_bytes() const { return urx::depth::resident_bytes(entries, n_ref, text_runs()); }
int DepthBeside::begin(uint32_t n) {
	out->records = n;
	return W.begin(n_ref, names, lens, entries);
}
int DepthBeside::count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) {
	return depth_count(W, at, base, off, i0, i1, action, min_mapq, stream);
}
int DepthBeside::finish() { return depth_finish(W, out); }
void DepthBeside::free_result() { urmapx_depth_free(out); }

}  // namespace depth
}  // namespace urx

extern "C" {

int urmapx_bam_depth(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint64_t *starts,
                     size_t n_starts, const urmapx_depth_opts *opts, urmapx_depth_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t entries = 0;
	int rc = check_refs(n_ref, names, lens, &entries);
	if (rc) return rc;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	try {
		t_alloc_s = 0;
		DepthBeside B(n_ref, names, lens, entries, opts ? opts->min_mapq : 0u, out);
		rc = staged_alone(device, (const uint8_t *)records, n_bytes, n_ref, starts, n_starts, B, &out->stage_chunks, &out->count_s);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	out->alloc_s = t_alloc_s;  // (the arrays are freed by now)
	if (rc) urmapx_depth_free(out);
	return rc;
}

}  // extern "C"
