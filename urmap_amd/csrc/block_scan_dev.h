// block_scan_dev.h -- the one-workgroup exclusive scan of 32-bit counts that the depth (depth.hip) and the pileup (pileup.hip) both put
// between a counting and a writing kernel.  HIP translation units only.  Not installed.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace urx {
namespace devscan {

constexpr uint32_t BS_NT = 1024;  // threads of block_scan_kernel

// one workgroup: out[i] = in[0] + .. + in[i - 1] for i < m (out may be in), the total to out[m] if with_total
template <class TO>
__global__ __launch_bounds__(BS_NT) void block_scan_kernel(const uint32_t *in, TO *out, uint32_t m, int with_total) {
	__shared__ uint64_t part[BS_NT];
	const uint32_t t = threadIdx.x, run = (m + BS_NT - 1) / BS_NT;
	const uint64_t lo = (uint64_t)t * run < m ? (uint64_t)t * run : m, hi = lo + run < m ? lo + run : m;
	uint64_t sum = 0;
	for (uint64_t i = lo; i < hi; ++i) sum += in[i];
	part[t] = sum;
	__syncthreads();
	for (uint32_t s = 1; s < BS_NT; s <<= 1) {
		const uint64_t a = t >= s ? part[t - s] : 0;
		__syncthreads();
		part[t] += a;
		__syncthreads();
	}
	uint64_t at = part[t] - sum;
	for (uint64_t i = lo; i < hi; ++i) {
		const uint32_t x = in[i];
		out[i] = (TO)at;
		at += x;
	}
	if (with_total && t == BS_NT - 1) out[m] = (TO)part[t];
}

}  // namespace devscan
}  // namespace urx
