// Where does one global_load_lds_dwordx3 put each lane's three dwords in LDS?  One wave, a known source pattern, the whole LDS array dumped.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ void glds_dwordx3(const void *gsrc, uint32_t lds_dst) {
	unsigned keep;
	asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx3 %1, off\n\ts_mov_b32 m0, %0"
	             : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__global__ __launch_bounds__(64) void probe(const uint32_t *src, uint32_t *out, int dword_off) {
	__shared__ __attribute__((aligned(16))) uint32_t a[1024];
	const int lane = threadIdx.x;
	for (int i = lane; i < 1024; i += 64) a[i] = 0xEEEE0000u + i;
	__syncthreads();
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	glds_dwordx3(src + 4 * lane, uni((uint32_t)(uintptr_t)(a + dword_off)));
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	for (int i = lane; i < 1024; i += 64) out[i] = a[i];
}
int main() {
	std::vector<uint32_t> h(64 * 4);
	for (int l = 0; l < 64; ++l) for (int k = 0; k < 4; ++k) h[4 * l + k] = (l << 8) | k;  // lane << 8 | dword
	uint32_t *d_src, *d_out;
	if (hipMalloc(&d_src, h.size() * 4) != hipSuccess || hipMalloc(&d_out, 4096) != hipSuccess) return 2;
	hipMemcpy(d_src, h.data(), h.size() * 4, hipMemcpyHostToDevice);
	for (int off : {0, 257}) {
		hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d_src, d_out, off);
		std::vector<uint32_t> o(1024);
		if (hipMemcpy(o.data(), d_out, 4096, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 3; }
		printf("== destination a + %d dwords: dwords that changed (index relative to the destination: value = lane << 8 | source dword)\n", off);
		int n = 0;
		for (int i = 0; i < 1024; ++i) if (o[i] != 0xEEEE0000u + i) { printf("%d:%x ", i - off, o[i]); if (++n % 16 == 0) printf("\n"); }
		printf("\n%d dwords written\n", n);
	}
	return 0;
}
