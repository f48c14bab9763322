// ufi_stats.hip -- the index statistics of -ufi_stats / -ufi_counts (ufistats.cpp:5-124, ufindex.cpp:338-456, 551-577) over a
// resident table, as two device passes.
//
// The reference makes five single-threaded passes: CountSlots and CountSlots_Minus over the sequence (a saturating byte per
// slot: how many words hash there, on the plus strand and as reverse complements), CountIndexedWords over it again (is each
// word's start position in its slot's row?), then LogStats and GetCollisionCount over every slot.  Here:
//   position pass  one thread per position of [0, SeqDataSize - 1) (FromFile's m_EndPos: the last byte is never looked at), the
//                  block's bytes staged in LDS: the word that ENDS at the position (Wildcard if it is not complete), its plus count,
//                  the reverse complement of the same window into the minus counts, and the Indexed test: a walk of the slot's row
//                  (walk_row, dev_common.h: GetRow with the MaxIx cap and long links) looking for the word's start;
//   slot pass      one thread per slot: tally classes, the row (K, Indexed2, and Collision: entries whose W raw bytes differ from
//                  entry 0's), CountHist / TruncHist from the two count arrays.  LDS histograms, one 64-bit atomic per block and bin.
// Counters are 64 bit (the reference's are 32-bit `unsigned`).  Slot numbers and offsets are 64 bit, and the blocks loop over the
// groups, so tables of more than 2^32 slots work.  A damaged row (K >= 256, or a position at or past the sequence store that the
// reference would memcmp) is never used to read the sequence: the pass counts it and reports the lowest such slot.
#include "kernels.h"

#include "dev_common.h"

#include <vector>

namespace urx {

static constexpr int ST_BLOCK = 256;
static constexpr int ST_HALO = 32;  // the longest word this pass takes

// ++counts[slot], saturating at 255, on the 32-bit word that holds the byte: a compare-and-swap, so a neighbour never sees a carry.
// Skipped once the byte reads 255 (hot slots: the repeat families of a genome hash their copies to one slot).
__device__ __forceinline__ void sat_inc(uint8_t *counts, uint64_t slot) {
	uint32_t *w = reinterpret_cast<uint32_t *>(counts + (slot & ~3ull));
	const uint32_t sh = 8u * (uint32_t)(slot & 3ull);
	uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	while (((old >> sh) & 0xFFu) != 0xFFu) {
		const uint32_t prev = atomicCAS(w, old, old + (1u << sh));
		if (prev == old) break;
		old = prev;
	}
}

// row cap of the walks: MaxIx, or 256 where the header's MaxIx does not bound a row the reference can hold (K >= 256 is damage)
__device__ __forceinline__ uint32_t row_cap(uint32_t maxIx) { return maxIx >= 1u && maxIx < 256u ? maxIx : 256u; }

// counters of the position pass
enum { PC_INDEXED, PC_NOT_INDEXED, PC_WILDCARD, PC_WORDS };

__global__ __launch_bounds__(ST_BLOCK) void stats_position_kernel(DevIndex X, uint32_t end, uint8_t *__restrict__ plus, uint8_t *__restrict__ minus,
                                                                  int indexed_test, unsigned long long *__restrict__ out, uint32_t tiles) {
	__shared__ uint8_t tile[ST_HALO + ST_BLOCK];
	__shared__ unsigned long long acc[PC_WORDS];
	if (threadIdx.x < PC_WORDS) acc[threadIdx.x] = 0;
	const uint32_t W = X.W, cap = row_cap(X.maxIx);
	const uint64_t N = X.slotCount;
	unsigned long long indexed = 0, not_indexed = 0, wildcard = 0;
	for (uint32_t g = blockIdx.x; g < tiles; g += gridDim.x) {
		const uint64_t base = (uint64_t)g * ST_BLOCK;
		__syncthreads();
		// bytes [base - 32, base + 256) of [0, end); outside it: 0, no letter
		for (uint32_t j = threadIdx.x; j < ST_HALO + ST_BLOCK; j += ST_BLOCK) {
			const int64_t at = (int64_t)base - ST_HALO + (int64_t)j;
			tile[j] = (at >= 0 && at < (int64_t)end) ? X.seq[at] : (uint8_t)0;
		}
		__syncthreads();
		const uint64_t t = base + threadIdx.x;  // the position: the word that ends here
		if (t >= end) continue;
		bool fwd_ok = t + 1 >= W, rev_ok = fwd_ok;
		uint64_t fwd = 0, rev = 0;
		for (uint32_t i = 0; i < W && fwd_ok; ++i) {
			const uint32_t c = tile[threadIdx.x + ST_HALO + 1 - W + i];
			const uint32_t L = letter_of(c);
			fwd_ok = L < 4u;
			rev_ok = rev_ok && c != 'u';  // g_CharToCompLetter has no 'u' (alpha.cpp:3525); g_CharToLetterNucleo does
			fwd = (fwd << 2) | (L & 3u);
			rev |= (uint64_t)(3u - (L & 3u)) << (2 * i);
		}
		if (!fwd_ok) { ++wildcard; continue; }
		const uint64_t slot = mod_slots(murmur64(fwd & X.shiftMask), N, X.slotMagic);
		if (plus) sat_inc(plus, slot);
		if (minus && rev_ok) sat_inc(minus, mod_slots(murmur64(rev & X.shiftMask), N, X.slotMagic));
		if (!indexed_test) continue;
		uint32_t T, pos;
		load_slot(X.blob, slot, T, pos);
		bool found = false;
		if (T & TALLY_MY_BIT) {
			const uint32_t start = (uint32_t)(t + 1 - W);
			(void)walk_row(X.blob, N, cap, slot, T, pos, [&](uint32_t, uint32_t p) { found = found || p == start; });
		}
		if (found) ++indexed;
		else ++not_indexed;
	}
	__syncthreads();
	if (indexed) atomicAdd(&acc[PC_INDEXED], indexed);
	if (not_indexed) atomicAdd(&acc[PC_NOT_INDEXED], not_indexed);
	if (wildcard) atomicAdd(&acc[PC_WILDCARD], wildcard);
	__syncthreads();
	if (threadIdx.x < PC_WORDS && acc[threadIdx.x]) atomicAdd(out + threadIdx.x, acc[threadIdx.x]);
}

// counters of the slot pass, in urmapx_ufi_stats order from `indexed2`
enum {
	SC_INDEXED2, SC_FREE, SC_COLLISION, SC_SINGLE_BOTH, SC_SINGLE_PLUS, SC_END, SC_MINE, SC_OTHER, SC_TRUNC, SC_TRUNC2, SC_LONG_MINE,
	SC_LONG_OTHER, SC_TOTAL, SC_BAD_ROWS, SC_WORDS
};

__global__ __launch_bounds__(ST_BLOCK) void stats_slot_kernel(DevIndex X, const uint8_t *__restrict__ plus, const uint8_t *__restrict__ minus,
                                                              unsigned long long *__restrict__ out, unsigned long long *__restrict__ hist,
                                                              unsigned long long *__restrict__ first_bad, uint32_t groups) {
	__shared__ uint32_t h_count[256], h_trunc[256];
	__shared__ unsigned long long acc[SC_WORDS];
	for (uint32_t i = threadIdx.x; i < 256; i += ST_BLOCK) h_count[i] = h_trunc[i] = 0;
	if (threadIdx.x < SC_WORDS) acc[threadIdx.x] = 0;
	__syncthreads();
	unsigned long long c[SC_WORDS];  // (constant indices only: registers)
#pragma unroll
	for (int i = 0; i < SC_WORDS; ++i) c[i] = 0;
	unsigned long long bad_slot = ~0ull;
	const uint64_t N = X.slotCount;
	const uint32_t W = X.W, cap = row_cap(X.maxIx), sds = X.seqDataSize;
	for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
		const uint64_t s = (uint64_t)g * ST_BLOCK + threadIdx.x;
		if (s >= N) continue;
		uint32_t T, pos;
		load_slot(X.blob, s, T, pos);
		c[SC_FREE] += T == TALLY_FREE;
		c[SC_SINGLE_PLUS] += T == TALLY_PLUS1;
		c[SC_SINGLE_BOTH] += T == TALLY_BOTH1;
		c[SC_END] += T == TALLY_END;
		c[SC_LONG_MINE] += T == TALLY_LONG_MINE;
		c[SC_LONG_OTHER] += T == TALLY_LONG_OTHER;
		c[SC_MINE] += (T & TALLY_MY_BIT) != 0;
		c[SC_OTHER] += T != TALLY_FREE && (T & TALLY_MY_BIT) == 0;
		uint32_t K = 0;
		if (T & TALLY_MY_BIT) {
			// GetCollisionCount: entries k >= 1 whose W bytes differ from entry 0's.  Every entry is checked against the sequence store
			// before any byte is read; the reference asserts there (and on K >= 256)
			uint32_t p0 = 0, collisions = 0;
			bool bad = false;
			K = walk_row(X.blob, N, cap, s, T, pos, [&](uint32_t k, uint32_t p) {
				if (k == 0) { p0 = p; return; }
				if (p >= sds || p0 >= sds) { bad = true; return; }
				if (bad) return;
				const uint8_t *a = X.seq + p, *b = X.seq + p0;  // (the store is padded: W bytes from a position inside it are readable)
				uint32_t i = 0;
				while (i < W && a[i] == b[i]) ++i;
				collisions += i < W;
			});
			if (K >= 256u) bad = true;
			if (bad) {
				++c[SC_BAD_ROWS];
				if (s < bad_slot) bad_slot = s;
			} else
				c[SC_COLLISION] += collisions;
		}
		c[SC_INDEXED2] += K;
		const uint32_t n = plus[s], nm = minus[s];
		atomicAdd(&h_count[n], 1u);
		c[SC_TOTAL] += n;
		if (n > 0 && K < n && n <= X.maxIx && nm <= X.maxIx) {
			++c[SC_TRUNC2];
			c[SC_TRUNC] += n;
			atomicAdd(&h_trunc[n], 1u);
		}
	}
#pragma unroll
	for (int i = 0; i < SC_WORDS; ++i)
		if (c[i]) atomicAdd(&acc[i], c[i]);
	if (bad_slot != ~0ull) atomicMin(first_bad, bad_slot);
	__syncthreads();
	if (threadIdx.x < SC_WORDS && acc[threadIdx.x]) atomicAdd(out + threadIdx.x, acc[threadIdx.x]);
	for (uint32_t i = threadIdx.x; i < 256; i += ST_BLOCK) {
		if (h_count[i]) atomicAdd(hist + i, (unsigned long long)h_count[i]);
		if (h_trunc[i]) atomicAdd(hist + 256 + i, (unsigned long long)h_trunc[i]);
	}
}

static unsigned grid_of(uint64_t groups) { return (unsigned)(groups < 65536 ? groups : 65536); }

// the two count arrays, slot_count bytes each (rounded up to whole 32-bit words for the compare-and-swap), zeroed
static hipError_t alloc_counts(uint64_t slot_count, uint8_t **p) {
	*p = nullptr;
	const uint64_t bytes = (slot_count + 7) & ~3ull;
	hipError_t e = hipMalloc((void **)p, bytes);
	if (e != hipSuccess) { *p = nullptr; return e; }
	return hipMemset(*p, 0, bytes);
}

static hipError_t launch_position(const DevIndex &X, uint8_t *plus, uint8_t *minus, int indexed_test, unsigned long long *d_out) {
	const uint32_t end = X.seqDataSize ? X.seqDataSize - 1u : 0u;  // FromFile: m_EndPos = SeqDataSize - 1 (ufindexio.cpp:70-71)
	const uint64_t tiles = ((uint64_t)end + ST_BLOCK - 1) / ST_BLOCK;
	if (tiles == 0) return hipSuccess;
	hipLaunchKernelGGL(stats_position_kernel, dim3(grid_of(tiles)), dim3(ST_BLOCK), 0, nullptr, X, end, plus, minus, indexed_test, d_out, (uint32_t)tiles);
	return hipGetLastError();
}

hipError_t ufi_stats_device(const DevIndex &X, uint64_t counters[UFI_STATS_COUNTERS], uint64_t hist[512], uint64_t *first_bad_slot, float ms[2]) {
	if (X.W < 1 || X.W > (uint32_t)ST_HALO || X.slotCount == 0) return hipErrorInvalidValue;
	const uint64_t groups = (X.slotCount + ST_BLOCK - 1) / ST_BLOCK;
	if (groups > 0xFFFFFFFFull) return hipErrorInvalidValue;
	uint8_t *plus = nullptr, *minus = nullptr;
	unsigned long long *d = nullptr;  // PC_WORDS position counters, SC_WORDS slot counters, first bad slot, 512 histogram bins
	const size_t n_words = PC_WORDS + SC_WORDS + 1 + 512;
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	hipError_t e = alloc_counts(X.slotCount, &plus);
	if (e == hipSuccess) e = alloc_counts(X.slotCount, &minus);
	if (e == hipSuccess) e = hipMalloc((void **)&d, n_words * 8);
	if (e == hipSuccess) e = hipMemset(d, 0, n_words * 8);
	if (e == hipSuccess) e = hipMemset(d + PC_WORDS + SC_WORDS, 0xFF, 8);
	for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
	if (e == hipSuccess) e = hipEventRecord(ev[0], nullptr);
	if (e == hipSuccess) e = launch_position(X, plus, minus, 1, d);
	if (e == hipSuccess) e = hipEventRecord(ev[1], nullptr);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(stats_slot_kernel, dim3(grid_of(groups)), dim3(ST_BLOCK), 0, nullptr, X, plus, minus, d + PC_WORDS, d + PC_WORDS + SC_WORDS + 1,
		                   d + PC_WORDS + SC_WORDS, (uint32_t)groups);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipEventRecord(ev[2], nullptr);
	std::vector<unsigned long long> h(n_words, 0);
	if (e == hipSuccess) e = hipMemcpy(h.data(), d, n_words * 8, hipMemcpyDeviceToHost);
	if (e == hipSuccess) {
		(void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
		(void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
		for (int i = 0; i < PC_WORDS + SC_WORDS; ++i) counters[i] = h[i];
		*first_bad_slot = h[PC_WORDS + SC_WORDS];
		for (int i = 0; i < 512; ++i) hist[i] = h[PC_WORDS + SC_WORDS + 1 + i];
	}
	for (hipEvent_t x : ev)
		if (x) (void)hipEventDestroy(x);
	(void)hipFree(plus); (void)hipFree(minus); (void)hipFree(d);
	return e;
}

hipError_t ufi_slot_counts_device(const DevIndex &X, int minus, uint8_t *host_out) {
	if (X.W < 1 || X.W > (uint32_t)ST_HALO || X.slotCount == 0) return hipErrorInvalidValue;
	uint8_t *counts = nullptr;
	unsigned long long *d = nullptr;
	hipError_t e = alloc_counts(X.slotCount, &counts);
	if (e == hipSuccess) e = hipMalloc((void **)&d, PC_WORDS * 8);
	if (e == hipSuccess) e = hipMemset(d, 0, PC_WORDS * 8);
	if (e == hipSuccess) e = launch_position(X, minus ? nullptr : counts, minus ? counts : nullptr, 0, d);
	if (e == hipSuccess) e = hipMemcpy(host_out, counts, X.slotCount, hipMemcpyDeviceToHost);
	(void)hipFree(counts); (void)hipFree(d);
	return e;
}

}  // namespace urx
