// markdup.hip -- duplicate marking on the device (urmapx_bam_sort_markdup; the rule is in include/urmapx.h "Duplicate marking"): bit
// 0x400 of the records that lie in HBM for the coordinate sort, written before gather_kernel copies them into order.  It runs inside
// DeviceSort::mark_duplicates (bam_sort.hip) in arrays the sort has used up, and sorts with the sort's own radix_sort and scan_launch.
//
//   ends_kernel       one WAVEFRONT per record: the lanes sum the QUAL bytes 64 at a time and reduce across the wave, lane 0 walks the
//                     CIGAR for u5.  Per record: u5 (signed), the score, what the record is (eligible, strand)
//   range_kernel      smallest and largest u5 of the eligible records: they size the packed end
//   pack_kernel       the packed end: reference, then u5 - smallest, then strand -- an unsigned number that orders as the ends do
//   first_kernel      one thread per adjacent pair of records: is it a pair (flags, names)
//   pair_fill / pair_lo / pair_head / pair_best / pair_write
//                     the pairs' numbers sorted by the higher end, then (stable) by the lower; a flag where either changes, scanned
//                     into group numbers; atomicMax of (score, ~first record) per group; 0x400 of both records where the pair is not
//                     its group's best
//   frag_flag / frag_fill / frag_head / frag_best / frag_write
//                     all eligible records sorted by their end; groups as above; a member of a pair puts the largest word there is
//                     into its group, a fragment its (score, ~record): a fragment that is not its group's best is a duplicate
// A maximum does not depend on the order the atomics arrive in, so nothing here depends on scheduling.  Flag bytes are written with
// byte stores (a record starts at any address), each by the one thread that owns the record.
// Only ends_kernel and first_kernel read a record's bytes.  They take a chunk of records (markdup_chunk): the whole input where it
// is resident, a staged chunk of it on the sort's external road, where the decisions go to an action array instead of the records.
#include "bam_sort_dev.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace urx::bamsort;

namespace {

constexpr uint32_t ELIGIBLE = 1u, REVERSE = 2u;  // what[i]
constexpr uint32_t ST_MIN = 0, ST_MAX = 1, ST_BAD = 2, ST_PAIR_DUP = 3, ST_FRAG = 4, ST_FRAG_DUP = 5, ST_WORDS = 8;  // the statistics block (64-bit words)
constexpr unsigned long long PAIR_MEMBER = ~0ull;  // beats every fragment's word (a score is below 2^31)

__device__ __forceinline__ uint64_t sum64(uint64_t v) {  // the wave's sum, in every lane
	for (int d = 32; d; d >>= 1)
		v += (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
	return v;
}
__device__ __forceinline__ int64_t xor64(int64_t v, int d) {
	return (int64_t)((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d, 64) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64));
}
// What the threads of a workgroup have counted, added to *to by one of them: the wave's sum by shuffles, the four waves' through a word of
// LDS (zero on entry, all threads of the workgroup call this together).  One atomic a workgroup on the counter -- atomics on one address
// queue up behind each other, and one a wavefront was 1.5 ms of frag_write_kernel at 4 M records
__device__ __forceinline__ void count_block(uint32_t mine, uint32_t *s_sum, unsigned long long *to) {
	for (int d = 32; d; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
	if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(s_sum, mine);
	__syncthreads();
	if (threadIdx.x == 0 && *s_sum) atomicAdd(to, (unsigned long long)*s_sum);
}
// what becomes of record v's bit 0x400: into the resident record, or -- where the records are not resident (action != nullptr) -- the same
// decision into the action array, which place_kernel (bam_sort.hip) applies as it copies the record
__device__ __forceinline__ void write_dup(uint8_t *rec, const uint64_t *off, uint8_t *action, uint32_t v, bool dup) {
	if (action) { action[v] = dup ? MD_SET : MD_CLEAR; return; }
	uint8_t *r = rec + off[v];
	const uint8_t b = r[FLAG_BYTE];
	r[FLAG_BYTE] = dup ? (uint8_t)(b | FLAG_DUP_BIT) : (uint8_t)(b & ~FLAG_DUP_BIT);
}

// The records i0 .. i1 - 1 lie at rec + (off[i] - base): a staged chunk whose first byte is byte `base` of the input, or (base 0, all
// records) the whole input.  word[i]: the score in the high half, refID in the low one -- what pack_kernel needs of a record's bytes
__global__ __launch_bounds__(NT) void ends_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, int64_t *u5, uint64_t *word,
                                                  uint32_t *what, unsigned long long *stat) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t wave = ((uint64_t)blockIdx.x * NT + threadIdx.x) >> 6, n_waves = (uint64_t)gridDim.x * (NT / 64);
	for (uint64_t i = i0 + wave; i < i1; i += n_waves) {  // (i is the same in all lanes of a wave)
		const uint8_t *r = rec + (off[i] - base);
		const uint64_t len = off[i + 1] - off[i];
		const uint32_t ref_id = load_u32(r + 4);
		const uint32_t w3 = load_u32(r + 12), w4 = load_u32(r + 16), l_seq = load_u32(r + 20);
		const uint32_t l_name = w3 & 0xFFu, n_cigar = w4 & 0xFFFFu, flag = w4 >> 16;
		if (flag & (0x4u | 0x100u | 0x800u)) {
			if (lane == 0) { what[i] = 0; word[i] = ref_id; u5[i] = 0; }
			continue;
		}
		const uint64_t qual_at = (uint64_t)CORE + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u;
		if (qual_at + l_seq > len) {  // SEQ and QUAL do not lie inside the record: the call is refused
			if (lane == 0) { what[i] = 0; word[i] = ref_id; u5[i] = 0; atomicOr(&stat[ST_BAD], 1ull); }
			continue;
		}
		const uint8_t *q = r + qual_at;
		uint64_t sum = 0;
		for (uint64_t k = lane; k < l_seq; k += 64u) {
			const uint32_t b = q[k];
			sum += b >= 15u && b != 0xFFu ? b : 0u;
		}
		sum = sum64(sum);
		if (lane == 0) {
			const uint8_t *c = r + CORE + l_name;  // (inside the record: scan_records has seen to it)
			const bool rev = flag & 0x10u;
			int64_t span = 0, front = 0, behind = 0;  // S and H in front of the first reference-consuming op; behind the last one
			bool seen = false;
			for (uint32_t k = 0; k < n_cigar; ++k) {
				const uint32_t w = load_u32(c + 4u * k), op = w & 15u;
				if (consumes_ref(op)) { span += w >> 4; seen = true; behind = 0; }
				else if (op == 4u || op == 5u) { if (!seen) front += w >> 4; behind += w >> 4; }
			}
			const int64_t pos = (int32_t)load_u32(r + 8);
			u5[i] = rev ? pos + (span ? span : 1) - 1 + behind : pos - front;
			word[i] = (uint64_t)(sum < MAX_SCORE ? (uint32_t)sum : MAX_SCORE) << 32 | ref_id;
			what[i] = ELIGIBLE | (rev ? REVERSE : 0u);
		}
	}
}

__global__ __launch_bounds__(NT) void range_kernel(const int64_t *u5, const uint32_t *what, uint32_t n, unsigned long long *stat) {
	int64_t lo = INT64_MAX, hi = INT64_MIN;
	for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT)
		if (what[i] & ELIGIBLE) { lo = u5[i] < lo ? u5[i] : lo; hi = u5[i] > hi ? u5[i] : hi; }
	for (int d = 32; d; d >>= 1) {
		const int64_t a = xor64(lo, d), b = xor64(hi, d);
		lo = a < lo ? a : lo; hi = b > hi ? b : hi;
	}
	if ((threadIdx.x & 63u) == 0 && lo <= hi) {
		atomicMin((long long *)&stat[ST_MIN], (long long)lo);
		atomicMax((long long *)&stat[ST_MAX], (long long)hi);
	}
}

// in place: u5 becomes the packed end (an ineligible record's stays unread); ends_kernel's words come apart: the scores to their array,
// refID into the end.  No record bytes are read here
__global__ __launch_bounds__(NT) void pack_kernel(const uint64_t *word, const uint32_t *what, uint32_t n, uint32_t n_ref, int64_t u5_min, uint32_t u5_bits,
                                                  uint64_t *end, uint32_t *score) {
	for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
		score[i] = (uint32_t)(word[i] >> 32);
		if (!(what[i] & ELIGIBLE)) continue;
		const uint32_t ref_id = (uint32_t)word[i];
		const uint64_t r = ref_id == 0xFFFFFFFFu ? n_ref : ref_id;
		end[i] = (r << u5_bits | (uint64_t)((int64_t)end[i] - u5_min)) << 1 | (what[i] & REVERSE ? 1u : 0u);
	}
}

// Is (i, i + 1) a pair?  The rule scans from the front and skips a record that was taken as a second mate; here every i is tested on
// its own.  The two agree: a first mate has 0x40 and not 0x80, a second mate has 0x80, so no record can be both -- the record i of a
// candidate (i, i + 1) is never the second mate of (i - 1, i), and its record i + 1 never the first mate of (i + 1, i + 2).  In
// 0x40 0x80 0x80 only (0, 1) is a candidate, in 0x40 0x40 0x80 only (1, 2), as in the scan.
// Records i0 .. i1 - 1 of a chunk as in ends_kernel, which has run on them and on record i1: a chunk that is not the last has its
// successor's first record staged behind it, so every adjacent pair of the input is tested once, by the chunk that holds its first record.
__global__ __launch_bounds__(NT) void first_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, const uint32_t *what, uint32_t i0, uint32_t i1, uint32_t n,
                                                   uint32_t *first) {
	for (uint64_t i = (uint64_t)i0 + blockIdx.x * NT + threadIdx.x; i < i1; i += gridDim.x * NT) {
		bool pair = false;
		if (i + 1u < n && (what[i] & ELIGIBLE) && (what[i + 1] & ELIGIBLE)) {
			const uint8_t *a = rec + (off[i] - base), *b = rec + (off[i + 1] - base);
			const uint32_t fa = load_u32(a + 16) >> 16, fb = load_u32(b + 16) >> 16;
			const uint32_t la = a[12], lb = b[12];
			if ((fa & 0xC1u) == 0x41u && (fb & 0x81u) == 0x81u && la == lb) {
				pair = true;
				for (uint32_t k = 0; k < la; ++k)  // (inside both records: scan_records has seen to it)
					if (a[CORE + k] != b[CORE + k]) { pair = false; break; }
			}
		}
		first[i] = pair;
	}
}

__device__ __forceinline__ uint64_t hi_end(const uint64_t *end, uint32_t v) { return end[v] > end[v + 1] ? end[v] : end[v + 1]; }
__device__ __forceinline__ uint64_t lo_end(const uint64_t *end, uint32_t v) { return end[v] < end[v + 1] ? end[v] : end[v + 1]; }
__device__ __forceinline__ unsigned long long word_of(uint32_t score, uint32_t v) { return (unsigned long long)score << 32 | (uint32_t)~v; }

// ---- pairs ----
// index: pairs in front of i.  The pair's number is its first record's
__global__ __launch_bounds__(NT) void pair_fill_kernel(const uint32_t *first, const uint32_t *index, const uint64_t *end, uint32_t n, uint32_t n_pairs, uint64_t *key,
                                                       uint32_t *val) {
	for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT)
		if (first[i] && index[i] < n_pairs) { key[index[i]] = hi_end(end, i); val[index[i]] = i; }
}
__global__ __launch_bounds__(NT) void pair_lo_kernel(const uint32_t *val, const uint64_t *end, uint32_t n_pairs, uint64_t *key) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_pairs; j += gridDim.x * NT) key[j] = lo_end(end, val[j]);
}
__global__ __launch_bounds__(NT) void pair_head_kernel(const uint32_t *val, const uint64_t *end, uint32_t n_pairs, uint32_t *flag) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_pairs; j += gridDim.x * NT)
		flag[j] = j == 0 || lo_end(end, val[j]) != lo_end(end, val[j - 1]) || hi_end(end, val[j]) != hi_end(end, val[j - 1]);
}
// (index: groups that begin in front of j, so index + flag - 1 is j's group)
__global__ __launch_bounds__(NT) void pair_best_kernel(const uint32_t *val, const uint32_t *flag, const uint32_t *index, const uint32_t *score, uint32_t n_pairs,
                                                       unsigned long long *best) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_pairs; j += gridDim.x * NT) {
		const uint32_t g = index[j] + flag[j] - 1u, v = val[j];
		if (g < n_pairs) atomicMax(&best[g], word_of(score[v] + score[v + 1], v));
	}
}
__global__ __launch_bounds__(NT) void pair_write_kernel(const uint32_t *val, const uint32_t *flag, const uint32_t *index, const uint32_t *score, uint32_t n_pairs,
                                                        const unsigned long long *best, const uint64_t *off, uint8_t *rec, uint8_t *action, unsigned long long *stat) {
	__shared__ uint32_t s_dups;
	if (threadIdx.x == 0) s_dups = 0;
	__syncthreads();
	uint32_t dups = 0;
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_pairs; j += gridDim.x * NT) {
		const uint32_t g = index[j] + flag[j] - 1u, v = val[j];
		const bool dup = g < n_pairs && best[g] != word_of(score[v] + score[v + 1], v);
		write_dup(rec, off, action, v, dup);
		write_dup(rec, off, action, v + 1u, dup);
		dups += dup;
	}
	count_block(dups, &s_dups, &stat[ST_PAIR_DUP]);
}

// ---- fragments: all eligible records by their end ----
__global__ __launch_bounds__(NT) void frag_flag_kernel(const uint32_t *what, uint32_t n, uint32_t *flag) {
	for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) flag[i] = what[i] & ELIGIBLE;
}
__global__ __launch_bounds__(NT) void frag_fill_kernel(const uint32_t *what, const uint32_t *index, const uint64_t *end, uint32_t n, uint32_t n_elig, uint64_t *key,
                                                       uint32_t *val) {
	for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT)
		if ((what[i] & ELIGIBLE) && index[i] < n_elig) { key[index[i]] = end[i]; val[index[i]] = i; }
}
__global__ __launch_bounds__(NT) void frag_head_kernel(const uint64_t *key, uint32_t n_elig, uint32_t *flag) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_elig; j += gridDim.x * NT) flag[j] = j == 0 || key[j] != key[j - 1];
}
__device__ __forceinline__ bool in_pair(const uint32_t *first, uint32_t v) { return first[v] || (v && first[v - 1]); }
__global__ __launch_bounds__(NT) void frag_best_kernel(const uint32_t *val, const uint32_t *flag, const uint32_t *index, const uint32_t *score, const uint32_t *first,
                                                       uint32_t n_elig, unsigned long long *best) {
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_elig; j += gridDim.x * NT) {
		const uint32_t g = index[j] + flag[j] - 1u, v = val[j];
		if (g < n_elig) atomicMax(&best[g], in_pair(first, v) ? PAIR_MEMBER : word_of(score[v], v));
	}
}
__global__ __launch_bounds__(NT) void frag_write_kernel(const uint32_t *val, const uint32_t *flag, const uint32_t *index, const uint32_t *score, const uint32_t *first,
                                                        uint32_t n_elig, const unsigned long long *best, const uint64_t *off, uint8_t *rec, uint8_t *action,
                                                        unsigned long long *stat) {
	__shared__ uint32_t s_frags, s_dups;
	if (threadIdx.x == 0) s_frags = s_dups = 0;
	__syncthreads();
	uint32_t frags = 0, dups = 0;
	for (uint32_t j = blockIdx.x * NT + threadIdx.x; j < n_elig; j += gridDim.x * NT) {
		const uint32_t g = index[j] + flag[j] - 1u, v = val[j];
		if (in_pair(first, v)) continue;
		const bool dup = g < n_elig && best[g] != word_of(score[v], v);
		write_dup(rec, off, action, v, dup);
		++frags;
		dups += dup;
	}
	count_block(frags, &s_frags, &stat[ST_FRAG]);
	count_block(dups, &s_dups, &stat[ST_FRAG_DUP]);
}

}  // namespace

namespace urx {
namespace bamsort {

int MarkdupOwn::begin(uint32_t n) {
	int rc;
	if ((rc = end.alloc(n)) || (rc = best.alloc((size_t)n + 1)) || (rc = what.alloc(n)) || (rc = first.alloc(n)) || (rc = stat.alloc(ST_WORDS))) return rc;
	unsigned long long s[ST_WORDS] = {0};
	s[ST_MIN] = (unsigned long long)INT64_MAX;
	s[ST_MAX] = (unsigned long long)INT64_MIN;
	HIP_TRY(hipMemcpy(stat.p, s, sizeof s, hipMemcpyHostToDevice));
	return URMAPX_OK;
}

int markdup_chunk(const MarkdupOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, uint32_t n, hipStream_t stream) {
	if (i1 <= i0) return URMAPX_OK;
	const uint32_t seen = i1 < n ? i1 + 1u : n;  // (the successor's first record is staged behind the chunk: first_kernel looks at it)
	hipLaunchKernelGGL(ends_kernel, dim3(grid_for((uint64_t)(seen - i0) * 64u)), dim3(NT), 0, stream, rec, base, off, i0, seen, (int64_t *)W.end.p, W.best.p, W.what.p,
	                   W.stat.p);
	hipLaunchKernelGGL(first_kernel, dim3(grid_for(i1 - i0)), dim3(NT), 0, stream, rec, base, off, (const uint32_t *)W.what.p, i0, i1, n, W.first.p);
	HIP_TRY(hipGetLastError());
	return URMAPX_OK;
}

int markdup_device(const MarkdupArrays &A, const MarkdupOwn &W, urmapx_markdup_stats *md) {
	const uint32_t n = A.n;
	if (n == 0) return URMAPX_OK;
	const Dev<uint64_t> &d_end = W.end, &d_best = W.best;
	const Dev<uint32_t> &d_what = W.what, &d_first = W.first;
	const Dev<unsigned long long> &d_stat = W.stat;
	// URMAPX_VERBOSE: where the time goes, a line on stderr (scripts/markdup_bench.py reads it); the stream is waited for after each part
	const bool verbose = getenv("URMAPX_VERBOSE") != nullptr;
	double part_s[3] = {0, 0, 0};
	auto t0 = std::chrono::steady_clock::now();
	auto lap = [&](int k) {
		if (!verbose) return;
		(void)hipStreamSynchronize(nullptr);
		const auto t1 = std::chrono::steady_clock::now();
		part_s[k] += std::chrono::duration<double>(t1 - t0).count();
		t0 = t1;
	};
	unsigned long long stat[ST_WORDS] = {0};

	// ends, scores and pairs are there (markdup_chunk); the width of the packed end
	hipLaunchKernelGGL(range_kernel, dim3(grid_for(n, 1024)), dim3(NT), 0, nullptr, (const int64_t *)d_end.p, (const uint32_t *)d_what.p, n, d_stat.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(stat, d_stat.p, sizeof stat, hipMemcpyDeviceToHost));
	if (stat[ST_BAD]) return URMAPX_E_FORMAT;
	const int64_t u5_min = (int64_t)stat[ST_MIN], u5_max = (int64_t)stat[ST_MAX];
	if (u5_min > u5_max) return URMAPX_OK;  // no eligible record: nothing is written
	const uint32_t u5_bits = bits_for((uint64_t)u5_max - (uint64_t)u5_min), end_bits = bits_for(A.n_ref) + u5_bits + 1u;
	if (end_bits > 64u) return URMAPX_E_FORMAT;
	hipLaunchKernelGGL(pack_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, (const uint64_t *)d_best.p, (const uint32_t *)d_what.p, n, A.n_ref, u5_min, u5_bits, d_end.p,
	                   A.score);

	lap(0);

	// pairs: their numbers by (lower end, higher end), the best of every group
	uint32_t n_pairs = 0;
	scan_launch<uint32_t, uint32_t>(d_first.p, n, A.val[1], A.sums);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpy(&n_pairs, A.val[1] + n, 4, hipMemcpyDeviceToHost));
	if (n_pairs > n / 2) return URMAPX_E_NODEVICE;
	if (n_pairs) {
		hipLaunchKernelGGL(pair_fill_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, (const uint32_t *)d_first.p, (const uint32_t *)A.val[1], (const uint64_t *)d_end.p, n,
		                   n_pairs, A.key[0], A.val[0]);
		SortArrays S{{A.key[0], A.key[1]}, {A.val[0], A.val[1]}, 0};  // (the scan in val[1] is used up)
		(void)radix_sort(S, n_pairs, end_bits, A.hist);
		hipLaunchKernelGGL(pair_lo_kernel, dim3(grid_for(n_pairs)), dim3(NT), 0, nullptr, (const uint32_t *)S.val[S.in], (const uint64_t *)d_end.p, n_pairs, S.key[S.in]);
		(void)radix_sort(S, n_pairs, end_bits, A.hist);
		const uint32_t *val = S.val[S.in];
		uint32_t *flag = (uint32_t *)S.key[1 - S.in], *index = flag + n_pairs;  // (2 n_pairs + 1 words in an array of 2 n + 4)
		hipLaunchKernelGGL(pair_head_kernel, dim3(grid_for(n_pairs)), dim3(NT), 0, nullptr, val, (const uint64_t *)d_end.p, n_pairs, flag);
		scan_launch<uint32_t, uint32_t>(flag, n_pairs, index, A.sums);
		HIP_TRY(hipMemsetAsync(d_best.p, 0, (size_t)n_pairs * 8, nullptr));
		hipLaunchKernelGGL(pair_best_kernel, dim3(grid_for(n_pairs)), dim3(NT), 0, nullptr, val, (const uint32_t *)flag, (const uint32_t *)index, (const uint32_t *)A.score,
		                   n_pairs, (unsigned long long *)d_best.p);
		hipLaunchKernelGGL(pair_write_kernel, dim3(grid_for(n_pairs)), dim3(NT), 0, nullptr, val, (const uint32_t *)flag, (const uint32_t *)index, (const uint32_t *)A.score,
		                   n_pairs, (const unsigned long long *)d_best.p, A.off, A.rec, A.action, d_stat.p);
		HIP_TRY(hipGetLastError());
	}

	lap(1);

	// fragments: the eligible records by their end
	uint32_t n_elig = 0;
	{
		uint32_t *flag = (uint32_t *)A.key[1];
		hipLaunchKernelGGL(frag_flag_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, (const uint32_t *)d_what.p, n, flag);
		scan_launch<uint32_t, uint32_t>(flag, n, A.val[1], A.sums);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(&n_elig, A.val[1] + n, 4, hipMemcpyDeviceToHost));
		if (n_elig > n) return URMAPX_E_NODEVICE;
	}
	if (n_elig) {
		hipLaunchKernelGGL(frag_fill_kernel, dim3(grid_for(n)), dim3(NT), 0, nullptr, (const uint32_t *)d_what.p, (const uint32_t *)A.val[1], (const uint64_t *)d_end.p, n,
		                   n_elig, A.key[0], A.val[0]);
		SortArrays S{{A.key[0], A.key[1]}, {A.val[0], A.val[1]}, 0};
		(void)radix_sort(S, n_elig, end_bits, A.hist);
		const uint32_t *val = S.val[S.in];
		uint32_t *flag = (uint32_t *)S.key[1 - S.in], *index = flag + n_elig;  // (2 n_elig + 1 words in an array of 2 n + 4)
		hipLaunchKernelGGL(frag_head_kernel, dim3(grid_for(n_elig)), dim3(NT), 0, nullptr, (const uint64_t *)S.key[S.in], n_elig, flag);
		scan_launch<uint32_t, uint32_t>(flag, n_elig, index, A.sums);
		HIP_TRY(hipMemsetAsync(d_best.p, 0, (size_t)n_elig * 8, nullptr));
		hipLaunchKernelGGL(frag_best_kernel, dim3(grid_for(n_elig)), dim3(NT), 0, nullptr, val, (const uint32_t *)flag, (const uint32_t *)index, (const uint32_t *)A.score,
		                   (const uint32_t *)d_first.p, n_elig, (unsigned long long *)d_best.p);
		hipLaunchKernelGGL(frag_write_kernel, dim3(grid_for(n_elig)), dim3(NT), 0, nullptr, val, (const uint32_t *)flag, (const uint32_t *)index, (const uint32_t *)A.score,
		                   (const uint32_t *)d_first.p, n_elig, (const unsigned long long *)d_best.p, A.off, A.rec, A.action, d_stat.p);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpy(stat, d_stat.p, sizeof stat, hipMemcpyDeviceToHost));
	lap(2);
	if (verbose)
		fprintf(stderr, "markdup parts: ends %.4f pairs %.4f fragments %.4f; records %u pairs %u eligible %u end_bits %u\n", part_s[0], part_s[1], part_s[2], n, n_pairs,
		        n_elig, end_bits);
	md->pairs_examined = n_pairs;
	md->pairs_duplicate = stat[ST_PAIR_DUP];
	md->fragments_examined = stat[ST_FRAG];
	md->fragments_duplicate = stat[ST_FRAG_DUP];
	return URMAPX_OK;
}

}  // namespace bamsort
}  // namespace urx
