// bitvec.hip -- the k-mer bit-vector read filter on the device: `urmap -make_bitvec`, `-search_bitvec`, `-search_bitvec2`
// (makebitvec.cpp, searchbitvec.cpp, searchbitvec2.cpp, bitvec.{h,cpp}).
//
// The table is 4^W bits (uint32 words, bit n = bit n&31 of word n>>5, which is the .bv file's byte layout), resident in HBM.
// Every kernel here works on chunks of 64 consecutive window starts, one per lane: the 64 + W - 1 bytes under a chunk are two
// coalesced byte loads per lane, and four ballots of each half turn them into 128-bit planes (letter bit 0, letter bit 1, "not a
// letter", "no complement letter") held in scalar registers.  A lane's window is then W bits of each plane at its own offset:
// validity is one mask test (no serial walk over invalid letters), the strand-1 word is the two planes interleaved and inverted
// (complemented letters, the first letter least significant), the strand-0 word the same of the bit-reversed windows.
//   build    one chunk per wave iteration over the whole concatenated store; atomicOr into the table (include pass), a second
//            launch on the same stream atomicAnd(~bit) (exclude pass).  A word is read first and the atomic issued only when it
//            would change the bit: repeats issue none.  Both passes are idempotent, so the table does not depend on scheduling.
//   popcount the table's set bits (the "included" / "excluded" counts).
//   search   one wave per read; chunks of strand 0, then of strand 1 only if strand 0 found nothing; the first chunk with a set
//            word ends the strand.  One verdict byte per read: 0 none, 1 forward, 2 reverse.

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dev_common.h"
#include "internal.h"
#include "sam.h"

bool urx_load_fasta_keep_case(const char *path, std::vector<std::string> &labels, std::vector<std::string> &seqs);  // make_ufi.cpp

using namespace urx;

struct urmapx_bitvec {
	int device = -1;
	uint32_t W = 0;
	uint64_t bytes = 0;  // 4^W / 8: the file's bits
	uint64_t alloc = 0;  // bytes allocated: a multiple of 16 (the popcount reads uint4), zero beyond `bytes`
	uint32_t *d_tbl = nullptr;
	unsigned long long *d_count = nullptr;
	hipStream_t st = nullptr;
	hipEvent_t ev[4] = {};  // build: include start / end, exclude end; search: start / end (ev[0], ev[3])
	float ms[3] = {};
	bool search_pending = false;
	DevBuf<uint8_t> d_bases, d_verd;  // urmapx_bitvec_search's staging
	DevBuf<uint64_t> d_offs;
};

namespace {

constexpr int BLOCK = 256;  // four waves

// W bits of the 128-bit plane (lo, hi) from bit i on (i < 64, i + W <= 128)
__device__ __forceinline__ uint32_t window_bits(uint64_t lo, uint64_t hi, uint32_t i, uint32_t mask) {
	const uint64_t x = i == 0 ? lo : (lo >> i) | (hi << (64u - i));
	return (uint32_t)x & mask;
}

struct Words {
	uint64_t f, r;  // strand 0 word of the window (first letter most significant), strand 1 word (its reverse complement)
	bool okf, okr;  // all W letters valid / all W complement letters valid
};

// c_lo = byte at chunk position `lane`, c_hi = byte at lane + 64 (0 past the sequence: not a letter).  Every lane of the wave must call.
__device__ __forceinline__ Words chunk_words(uint32_t c_lo, uint32_t c_hi, uint32_t lane, uint32_t W) {
	const uint32_t l_lo = letter_of(c_lo), l_hi = letter_of(c_hi);  // g_CharToLetterNucleo
	const uint64_t b0l = __ballot(l_lo & 1u), b0h = __ballot(l_hi & 1u);
	const uint64_t b1l = __ballot((l_lo >> 1) & 1u), b1h = __ballot((l_hi >> 1) & 1u);
	const uint64_t ifl = __ballot(l_lo > 3u), ifh = __ballot(l_hi > 3u);
	// g_CharToCompChar maps ACGTU / acgt to letters again and 'u' to '?' (dev_common.h comp_char): complement invalid = letter invalid or 'u'
	const uint64_t irl = __ballot(l_lo > 3u || c_lo == 'u'), irh = __ballot(l_hi > 3u || c_hi == 'u');
	const uint32_t m = (1u << W) - 1u;
	const uint32_t x0 = window_bits(b0l, b0h, lane, m), x1 = window_bits(b1l, b1h, lane, m);
	Words w;
	w.okf = window_bits(ifl, ifh, lane, m) == 0u;
	w.okr = window_bits(irl, irh, lane, m) == 0u;
	// letter j of the window at bits 2j, complemented (3 - l = l ^ 3): the word of the reverse complement, whose first letter is the
	// complement of the window's last
	w.r = ((spread32(x1) << 1) | spread32(x0)) ^ ((1ull << (2u * W)) - 1ull);
	const uint32_t sh = 32u - W;
	w.f = (spread32(__builtin_bitreverse32(x1) >> sh) << 1) | spread32(__builtin_bitreverse32(x0) >> sh);
	return w;
}

template <bool CLEAR>
__device__ __forceinline__ void touch(uint32_t *tbl, uint64_t word) {
	uint32_t *p = tbl + (word >> 5);
	const uint32_t bit = 1u << (word & 31u);
	const uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (!CLEAR) {
		if (!(cur & bit)) atomicOr(p, bit);
	} else {
		if (cur & bit) atomicAnd(p, ~bit);
	}
}

// Scan (makebitvec.cpp:6-70) over every sequence of the store: seq[offs[k] .. offs[k+1]), offs[0] = 0, offs[nseq] = total.
// Strand 0 words start at s = 0 .. L-2W+1 of a sequence; the strand-1 word whose reverse-complement start is L-W-s covers the
// same bytes as the window at s, so strand 1 is the windows s = W-1 .. L-W.
template <bool CLEAR>
__global__ __launch_bounds__(BLOCK) void bv_build_kernel(const uint8_t *__restrict__ seq, const uint64_t *__restrict__ offs, uint32_t nseq,
                                                         uint64_t total, uint32_t W, uint32_t *__restrict__ tbl) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t nchunks = (total + 63u) / 64u;
	const uint64_t nwaves = (uint64_t)gridDim.x * (BLOCK / 64);
	for (uint64_t ch = (uint64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); ch < nchunks; ch += nwaves) {
		const uint64_t c0 = ch * 64u, q = c0 + lane;
		const uint32_t c_lo = q < total ? seq[q] : 0u;
		const uint32_t c_hi = q + 64u < total ? seq[q + 64u] : 0u;
		const Words w = chunk_words(c_lo, c_hi, lane, W);
		if (q < total && (w.okf || w.okr)) {
			// the sequence holding q: the last k with offs[k] <= q
			uint32_t lo = 0, hi = nseq;
			while (hi - lo > 1u) {
				const uint32_t mid = (lo + hi) >> 1;
				if (offs[mid] <= q) lo = mid;
				else hi = mid;
			}
			const uint64_t s = q - offs[lo], L = offs[lo + 1] - offs[lo];
			if (w.okf && s + 2u * W <= L + 1u) touch<CLEAR>(tbl, w.f);
			if (w.okr && s + 1u >= W && s + W <= L) touch<CLEAR>(tbl, w.r);
		}
	}
}

__global__ __launch_bounds__(BLOCK) void bv_popcount_kernel(const uint4 *__restrict__ tbl, uint64_t n16, unsigned long long *out) {
	unsigned long long c = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * BLOCK) {
		const uint4 v = tbl[i];
		c += (unsigned long long)(__builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w));
	}
	for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
	if ((threadIdx.x & 63u) == 0) atomicAdd(out, c);
}

// SearchBitVec1 (searchbitvec.cpp:17-55), one wave per read
__global__ __launch_bounds__(BLOCK) void bv_search_kernel(const uint32_t *__restrict__ tbl, uint32_t W, const uint8_t *__restrict__ bases,
                                                          const uint64_t *__restrict__ offs, uint32_t n, uint8_t *__restrict__ verdicts) {
	const uint32_t r = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
	if (r >= n) return;  // whole waves
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t b0 = offs[r], L = offs[r + 1] - b0;
	const uint8_t *read = bases + b0;
	uint32_t v = 0;
	if (L + 1u >= 2u * W) {
		const uint64_t nst = L + 2u - 2u * W;  // word starts per strand
		for (uint32_t strand = 0; strand < 2u && v == 0u; ++strand) {
			const uint64_t first = strand ? W - 1u : 0u;  // windows first .. first + nst - 1 of the read as given
			for (uint64_t c = 0; c < nst; c += 64u) {
				const uint64_t q = first + c + lane;
				const uint32_t c_lo = q < L ? read[q] : 0u;
				const uint32_t c_hi = q + 64u < L ? read[q + 64u] : 0u;
				const Words w = chunk_words(c_lo, c_hi, lane, W);
				bool hit = false;
				if (c + lane < nst && (strand ? w.okr : w.okf)) {
					const uint64_t word = strand ? w.r : w.f;
					hit = (tbl[word >> 5] >> (word & 31u)) & 1u;
				}
				if (__ballot(hit)) {
					v = strand + 1u;
					break;
				}
			}
		}
	}
	if (lane == 0) verdicts[r] = (uint8_t)v;
}

int grid_for(uint64_t items, uint64_t per_block, uint64_t cap) {
	return (int)std::max<uint64_t>(1, std::min<uint64_t>(cap, (items + per_block - 1) / per_block));
}

bool w_supported(uint32_t W) { return W >= URMAPX_BV_MIN_W && W <= URMAPX_BV_MAX_W; }

int bv_create(int device, uint32_t W, urmapx_bitvec **out) {
	*out = nullptr;
	if (!w_supported(W)) return URMAPX_E_UNSUPPORTED;
	urmapx_bitvec *B = new urmapx_bitvec;
	B->device = device;
	B->W = W;
	B->bytes = (1ull << (2 * W)) / 8u;
	B->alloc = (B->bytes + 15u) & ~15ull;
	hipError_t e = hipSetDevice(device);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&B->st, hipStreamNonBlocking);
	for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&B->ev[k]);
	if (e == hipSuccess) e = hipMalloc((void **)&B->d_count, sizeof(unsigned long long));
	if (e == hipSuccess) e = hipMalloc((void **)&B->d_tbl, B->alloc);
	if (e == hipSuccess) e = hipMemsetAsync(B->d_tbl, 0, B->alloc, B->st);
	if (e == hipSuccess) e = hipStreamSynchronize(B->st);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		urmapx_bitvec_close(B);
		return hip_rc(e);
	}
	*out = B;
	return URMAPX_OK;
}

// host sequences -> device store with offsets from 0
int upload_store(const uint8_t *seqs, const uint64_t *offs, uint32_t n, uint8_t **d_seq, uint64_t **d_offs, uint64_t *total) {
	*d_seq = nullptr; *d_offs = nullptr;
	const uint64_t base = offs[0], tot = offs[n] - offs[0];
	std::vector<uint64_t> o(n + 1);
	for (uint32_t i = 0; i <= n; ++i) {
		if (offs[i] < base || (i && offs[i] < offs[i - 1])) return URMAPX_E_ARG;
		o[i] = offs[i] - base;
	}
	HIP_TRY(hipMalloc((void **)d_offs, (n + 1) * sizeof(uint64_t)));
	HIP_TRY(hipMalloc((void **)d_seq, std::max<uint64_t>(tot, 1)));
	HIP_TRY(hipMemcpy(*d_offs, o.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
	if (tot) HIP_TRY(hipMemcpy(*d_seq, seqs + base, tot, hipMemcpyHostToDevice));
	*total = tot;
	return URMAPX_OK;
}

int popcount(const urmapx_bitvec *B, uint64_t *out) {
	HIP_TRY(hipSetDevice(B->device));
	HIP_TRY(hipMemsetAsync(B->d_count, 0, sizeof(unsigned long long), B->st));
	const uint64_t n16 = B->alloc / 16u;
	bv_popcount_kernel<<<grid_for(n16, 4 * BLOCK, 8192), BLOCK, 0, B->st>>>((const uint4 *)B->d_tbl, n16, B->d_count);
	HIP_TRY(hipGetLastError());
	unsigned long long c = 0;
	HIP_TRY(hipMemcpyAsync(&c, B->d_count, sizeof c, hipMemcpyDeviceToHost, B->st));
	HIP_TRY(hipStreamSynchronize(B->st));
	*out = c;
	return URMAPX_OK;
}

template <bool CLEAR>
int scan(urmapx_bitvec *B, const uint8_t *seqs, const uint64_t *offs, uint32_t n, hipEvent_t e0, hipEvent_t e1) {
	uint8_t *ds = nullptr;
	uint64_t *doff = nullptr, total = 0;
	int rc = upload_store(seqs, offs, n, &ds, &doff, &total);
	if (!rc) {
		if (hipEventRecord(e0, B->st) != hipSuccess) rc = URMAPX_E_NODEVICE;
		if (!rc && total) {
			bv_build_kernel<CLEAR><<<grid_for((total + 63) / 64, BLOCK / 64, 65536), BLOCK, 0, B->st>>>(ds, doff, n, total, B->W, B->d_tbl);
			rc = hip_rc(hipGetLastError());
		}
		if (!rc && hipEventRecord(e1, B->st) != hipSuccess) rc = URMAPX_E_NODEVICE;
		if (!rc) rc = hip_rc(hipStreamSynchronize(B->st));
	}
	if (ds) (void)hipFree(ds);
	if (doff) (void)hipFree(doff);
	return rc;
}

}  // namespace

extern "C" {

int urmapx_bitvec_build(int device, const uint8_t *seqs, const uint64_t *offs, uint32_t n, const uint8_t *excl, const uint64_t *excl_offs,
                        uint32_t n_excl, uint32_t W, urmapx_bitvec **out, uint64_t counts[2]) {
	if (!out || !offs || (n && !seqs) || (n_excl && (!excl || !excl_offs))) return URMAPX_E_ARG;
	*out = nullptr;
	urmapx_bitvec *B = nullptr;
	int rc = bv_create(device, W, &B);
	if (rc) return rc;
	uint64_t inc = 0, left = 0;
	rc = scan<false>(B, seqs, offs, n, B->ev[0], B->ev[1]);
	if (!rc) rc = popcount(B, &inc);
	if (!rc && n_excl) rc = scan<true>(B, excl, excl_offs, n_excl, B->ev[1], B->ev[2]);
	if (!rc) rc = n_excl ? popcount(B, &left) : URMAPX_OK;
	if (rc) { urmapx_bitvec_close(B); return rc; }
	if (!n_excl) left = inc;
	(void)hipEventElapsedTime(&B->ms[0], B->ev[0], B->ev[1]);
	if (n_excl) (void)hipEventElapsedTime(&B->ms[1], B->ev[1], B->ev[2]);
	if (counts) { counts[0] = inc; counts[1] = inc - left; }
	*out = B;
	return URMAPX_OK;
}

int urmapx_bitvec_open(const char *path, int device, urmapx_bitvec **out) {
	if (!path || !out) return URMAPX_E_ARG;
	*out = nullptr;
	FILE *f = fopen(path, "rb");
	if (!f) return URMAPX_E_IO;
	uint32_t hdr[2] = {0, 0};
	if (fread(hdr, 4, 2, f) != 2 || hdr[0] != URMAPX_BV_MAGIC) { fclose(f); return URMAPX_E_FORMAT; }
	urmapx_bitvec *B = nullptr;
	int rc = bv_create(device, hdr[1], &B);
	if (!rc) {
		int threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
		rc = stream_to_device(fileno(f), 8, B->bytes, (uint8_t *)B->d_tbl, threads);
	}
	fclose(f);
	if (rc) { urmapx_bitvec_close(B); return rc; }
	*out = B;
	return URMAPX_OK;
}

int urmapx_bitvec_wrap_host(int device, uint32_t W, const uint8_t *bits, urmapx_bitvec **out) {
	if (!bits || !out) return URMAPX_E_ARG;
	urmapx_bitvec *B = nullptr;
	int rc = bv_create(device, W, &B);
	if (rc) return rc;
	rc = hip_rc(hipMemcpy(B->d_tbl, bits, B->bytes, hipMemcpyHostToDevice));
	if (rc) { urmapx_bitvec_close(B); return rc; }
	*out = B;
	return URMAPX_OK;
}

int urmapx_bitvec_download(const urmapx_bitvec *B, uint8_t *bits, uint64_t cap) {
	if (!B || !bits || cap < B->bytes) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(B->device));
	HIP_TRY(hipMemcpy(bits, B->d_tbl, B->bytes, hipMemcpyDeviceToHost));
	return URMAPX_OK;
}

int urmapx_bitvec_save(const urmapx_bitvec *B, const char *path) {
	if (!B || !path) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(B->device));
	FILE *f = fopen(path, "wb");
	if (!f) return URMAPX_E_IO;
	const uint32_t hdr[2] = {URMAPX_BV_MAGIC, B->W};
	bool ok = fwrite(hdr, 4, 2, f) == 2;
	const uint64_t piece = std::min<uint64_t>(B->bytes, 64ull << 20);
	std::vector<uint8_t> buf(piece);
	int rc = URMAPX_OK;
	for (uint64_t off = 0; ok && !rc && off < B->bytes; off += piece) {
		const uint64_t k = std::min(piece, B->bytes - off);
		rc = hip_rc(hipMemcpy(buf.data(), (const uint8_t *)B->d_tbl + off, k, hipMemcpyDeviceToHost));
		if (!rc) ok = fwrite(buf.data(), 1, k, f) == k;
	}
	if (fclose(f) != 0) ok = false;
	if (rc) return rc;
	return ok ? URMAPX_OK : URMAPX_E_IO;
}

uint32_t urmapx_bitvec_word_length(const urmapx_bitvec *B) { return B ? B->W : 0u; }
uint64_t urmapx_bitvec_bytes(const urmapx_bitvec *B) { return B ? B->bytes : 0ull; }

int urmapx_bitvec_popcount(const urmapx_bitvec *B, uint64_t *out) {
	if (!B || !out) return URMAPX_E_ARG;
	return popcount(B, out);
}

int urmapx_bitvec_search_device(urmapx_bitvec *B, const void *d_bases, const void *d_offs, uint32_t n, void *d_verdicts) {
	if (!B || (n && (!d_bases || !d_offs || !d_verdicts))) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(B->device));
	HIP_TRY(hipEventRecord(B->ev[0], B->st));
	if (n)
		bv_search_kernel<<<(n + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, B->st>>>(B->d_tbl, B->W, (const uint8_t *)d_bases,
		                                                                           (const uint64_t *)d_offs, n, (uint8_t *)d_verdicts);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(B->ev[3], B->st));
	B->search_pending = true;
	return URMAPX_OK;
}

int urmapx_bitvec_sync(urmapx_bitvec *B) {
	if (!B) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(B->device));
	HIP_TRY(hipStreamSynchronize(B->st));
	if (B->search_pending) {
		(void)hipEventElapsedTime(&B->ms[2], B->ev[0], B->ev[3]);
		B->search_pending = false;
	}
	return URMAPX_OK;
}

int urmapx_bitvec_search(urmapx_bitvec *B, const uint8_t *bases, const uint64_t *offs, uint32_t n, uint8_t *verdicts) {
	if (!B || !offs || (n && (!bases || !verdicts))) return URMAPX_E_ARG;
	if (!n) return URMAPX_OK;
	HIP_TRY(hipSetDevice(B->device));
	const uint64_t base = offs[0], tot = offs[n] - offs[0];
	std::vector<uint64_t> o(n + 1);
	for (uint32_t i = 0; i <= n; ++i) {
		if (offs[i] < base || (i && offs[i] < offs[i - 1])) return URMAPX_E_ARG;
		o[i] = offs[i] - base;
	}
	int rc = B->d_bases.ensure(std::max<uint64_t>(tot, 1));
	if (!rc) rc = B->d_offs.ensure(n + 1);
	if (!rc) rc = B->d_verd.ensure(n);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(B->d_offs.p, o.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, B->st));
	if (tot) HIP_TRY(hipMemcpyAsync(B->d_bases.p, bases + base, tot, hipMemcpyHostToDevice, B->st));
	rc = urmapx_bitvec_search_device(B, B->d_bases.p, B->d_offs.p, n, B->d_verd.p);
	if (rc) return rc;
	HIP_TRY(hipMemcpyAsync(verdicts, B->d_verd.p, n, hipMemcpyDeviceToHost, B->st));
	return urmapx_bitvec_sync(B);
}

int urmapx_bitvec_last_ms(urmapx_bitvec *B, float ms[3]) {
	if (!B || !ms) return URMAPX_E_ARG;
	for (int k = 0; k < 3; ++k) ms[k] = B->ms[k];
	return URMAPX_OK;
}

void urmapx_bitvec_close(urmapx_bitvec *B) {
	if (!B) return;
	if (B->device >= 0) (void)hipSetDevice(B->device);
	if (B->st) (void)hipStreamSynchronize(B->st);
	B->d_bases.release();
	B->d_offs.release();
	B->d_verd.release();
	if (B->d_tbl) (void)hipFree(B->d_tbl);
	if (B->d_count) (void)hipFree(B->d_count);
	for (hipEvent_t e : B->ev)
		if (e) (void)hipEventDestroy(e);
	if (B->st) (void)hipStreamDestroy(B->st);
	delete B;
}

int urmapx_make_bitvec(int device, const char *ref_fa, const char *excl_fa, uint32_t W, const char *bv_path, uint64_t counts[2]) {
	if (!ref_fa || !excl_fa || !bv_path) return URMAPX_E_ARG;
	if (!w_supported(W)) return URMAPX_E_UNSUPPORTED;
	auto load = [](const char *path, std::vector<uint8_t> &store, std::vector<uint64_t> &offs) {
		std::vector<std::string> labels, seqs;
		if (!urx_load_fasta_keep_case(path, labels, seqs)) return false;
		offs.assign(1, 0);
		uint64_t total = 0;
		for (const std::string &s : seqs) total += s.size();
		store.resize(total);
		for (std::string &s : seqs) {
			memcpy(store.data() + offs.back(), s.data(), s.size());
			offs.push_back(offs.back() + s.size());
			std::string().swap(s);
		}
		return true;
	};
	std::vector<uint8_t> ref, excl;
	std::vector<uint64_t> ref_offs, excl_offs;
	if (!load(ref_fa, ref, ref_offs) || !load(excl_fa, excl, excl_offs)) return URMAPX_E_IO;
	urmapx_bitvec *B = nullptr;
	int rc = urmapx_bitvec_build(device, ref.data(), ref_offs.data(), (uint32_t)(ref_offs.size() - 1), excl.data(), excl_offs.data(),
	                             (uint32_t)(excl_offs.size() - 1), W, &B, counts);
	if (rc) return rc;
	rc = urmapx_bitvec_save(B, bv_path);
	urmapx_bitvec_close(B);
	return rc;
}

}  // extern "C"

// ---- file to file ----
namespace {

// one batch of reads (both mates' reads for pairs: mate 1 at [0, n), mate 2 at [n, 2n)) with its own copies of the text and the
// device arrays; two of them alternate so that batch b's copies and search run while batch b-1's records are written
struct Batch {
	std::vector<uint8_t> quals;
	std::vector<uint64_t> offs;  // n reads + 1, from 0
	std::vector<char> label_data;
	std::vector<uint64_t> label_offs;
	uint8_t *h_bases = nullptr, *h_verd = nullptr;  // page-locked
	size_t h_bases_cap = 0, h_verd_cap = 0;
	DevBuf<uint8_t> d_bases, d_verd;
	DevBuf<uint64_t> d_offs;
	hipEvent_t done = nullptr;
	uint32_t n = 0;  // reads
	bool busy = false;
	void clear() { quals.clear(); offs.assign(1, 0); label_data.clear(); label_offs.clear(); n = 0; }
	~Batch() {
		if (h_bases) (void)hipHostFree(h_bases);
		if (h_verd) (void)hipHostFree(h_verd);
		d_bases.release(); d_verd.release(); d_offs.release();
		if (done) (void)hipEventDestroy(done);
	}
};

int grow_pinned(uint8_t *&p, size_t &cap, size_t want) {
	if (want <= cap) return URMAPX_OK;
	if (p) (void)hipHostFree(p);
	p = nullptr; cap = 0;
	want = want + want / 4 + 4096;
	HIP_TRY(hipHostMalloc((void **)&p, want, hipHostMallocDefault));
	cap = want;
	return URMAPX_OK;
}

// append one reader batch (the arrays urmapx_fastq_next hands out) to b; bases go to the page-locked array at `at`
void take(Batch &b, uint32_t n, const uint8_t *bases, const uint8_t *quals, const uint64_t *offs, const char *label_data,
          const uint64_t *label_offs, uint64_t at) {
	const uint64_t nb = offs[n];
	memcpy(b.h_bases + at, bases, nb);
	b.quals.insert(b.quals.end(), quals, quals + nb);
	for (uint32_t i = 1; i <= n; ++i) b.offs.push_back(at + offs[i]);
	const uint64_t lbase = b.label_data.size();
	const uint64_t lbytes = n ? label_offs[n - 1] + strlen(label_data + label_offs[n - 1]) + 1 : 0;
	b.label_data.insert(b.label_data.end(), label_data, label_data + lbytes);
	for (uint32_t i = 0; i < n; ++i) b.label_offs.push_back(lbase + label_offs[i]);
	b.n += n;
}

// SeqInfo::ToFastq (seqinfo.cpp:408-426) of read i as SearchBitVec1 left it: verdict 1 = as read; 0 or 2 = reverse-complemented by
// characters (RevCompInPlace, seqinfo.cpp:327-360) with the quality string reversed.  Nothing for an empty read.
void append_record(std::string &out, const Batch &b, uint32_t i, bool trunc, const unsigned char *comp) {
	const uint64_t o = b.offs[i], L = b.offs[i + 1] - o;
	if (L == 0) return;
	const char *label = b.label_data.data() + b.label_offs[i];
	size_t ll = strlen(label);
	if (trunc)
		for (size_t k = 0; k < ll; ++k)
			if (isspace((unsigned char)label[k])) { ll = k; break; }
	out.push_back('@');
	out.append(label, ll);
	out.push_back('\n');
	const uint8_t *s = b.h_bases + o;
	const uint8_t *q = b.quals.data() + o;
	const size_t at = out.size();
	out.resize(at + 2 * L + 4);
	char *p = &out[at];
	if (b.h_verd[i] == 1) {
		memcpy(p, s, L);
		memcpy(p + L + 3, q, L);
	} else {
		for (uint64_t k = 0; k < L; ++k) {
			p[k] = (char)comp[s[L - 1 - k]];
			p[L + 3 + k] = (char)q[L - 1 - k];
		}
	}
	p[L] = '\n'; p[L + 1] = '+'; p[L + 2] = '\n';
	p[2 * L + 3] = '\n';
}

}  // namespace

extern "C" int urmapx_search_bitvec_files(urmapx_bitvec *B, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                          unsigned flags, uint64_t counts[2], char *err, size_t errcap) {
	auto fail = [&](int rc, const std::string &msg) {
		if (err && errcap) snprintf(err, errcap, "%s", msg.c_str());
		return rc;
	};
	if (err && errcap) err[0] = 0;
	const bool paired = fq2 != nullptr;
	if (!B || !fq1 || !out1 || (paired && !out2)) return fail(URMAPX_E_ARG, "missing file name");
	if (counts) counts[0] = counts[1] = 0;
	if (hipSetDevice(B->device) != hipSuccess) return fail(URMAPX_E_NODEVICE, "no usable GPU");
	urmapx_fastq *F1 = nullptr, *F2 = nullptr;
	if (urmapx_fastq_open(fq1, &F1)) return fail(URMAPX_E_IO, std::string("Cannot open ") + fq1);
	if (paired && urmapx_fastq_open(fq2, &F2)) { urmapx_fastq_close(F1); return fail(URMAPX_E_IO, std::string("Cannot open ") + fq2); }
	FILE *o1 = fopen(out1, "wb");
	FILE *o2 = paired ? fopen(out2, "wb") : nullptr;
	const unsigned char *comp = complement_table();
	const bool trunc = (flags & URMAPX_BV_TRUNC_LABELS) != 0;
	const uint32_t BATCH = paired ? (1u << 17) : (1u << 18);
	Batch bt[2];
	uint64_t found = 0, total = 0;
	int rc = URMAPX_OK;
	std::string msg;
	if (!o1 || (paired && !o2)) { rc = URMAPX_E_IO; msg = std::string("Cannot create ") + (!o1 ? out1 : out2); }
	for (Batch &b : bt)
		if (!rc && hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) rc = URMAPX_E_NODEVICE;
	// records of a searched batch, in input order
	auto write_batch = [&](Batch &b) -> int {
		HIP_TRY(hipEventSynchronize(b.done));
		b.busy = false;
		std::string t1, t2;
		const uint32_t np = paired ? b.n / 2 : b.n;
		for (uint32_t i = 0; i < np; ++i) {
			if (!paired) {
				if (b.h_verd[i]) { append_record(t1, b, i, trunc, comp); ++found; }
			} else if (b.h_verd[i] || b.h_verd[np + i]) {
				append_record(t1, b, i, trunc, comp);
				append_record(t2, b, np + i, trunc, comp);
				++found;
			}
		}
		total += np;
		if (fwrite(t1.data(), 1, t1.size(), o1) != t1.size() || (paired && fwrite(t2.data(), 1, t2.size(), o2) != t2.size())) return URMAPX_E_IO;
		return URMAPX_OK;
	};
	for (uint64_t k = 0; !rc; ++k) {
		Batch &b = bt[k & 1];
		if (b.busy && (rc = write_batch(b))) break;  // batch k-2's records (normally written already)
		b.clear();
		const uint8_t *bs1, *qs1, *bs2 = nullptr, *qs2 = nullptr;
		const uint64_t *of1, *of2 = nullptr, *lo1, *lo2 = nullptr;
		const char *ld1, *ld2 = nullptr;
		const int64_t n1 = urmapx_fastq_next(F1, BATCH, &bs1, &qs1, &of1, &ld1, &lo1);
		if (n1 < 0) { rc = URMAPX_E_FORMAT; msg = urmapx_fastq_error(F1); break; }
		int64_t n2 = 0;
		if (paired) {
			n2 = urmapx_fastq_next(F2, BATCH, &bs2, &qs2, &of2, &ld2, &lo2);
			if (n2 < 0) { rc = URMAPX_E_FORMAT; msg = urmapx_fastq_error(F2); break; }
			if (n2 != n1) { rc = URMAPX_E_FORMAT; msg = "-search_bitvec2: the two FASTQ files hold different numbers of records"; break; }
		}
		if (n1 == 0) break;
		const uint64_t nb = of1[n1] + (paired ? of2[n2] : 0);
		if ((rc = grow_pinned(b.h_bases, b.h_bases_cap, std::max<uint64_t>(nb, 1)))) break;
		if ((rc = grow_pinned(b.h_verd, b.h_verd_cap, (size_t)(n1 + n2)))) break;
		take(b, (uint32_t)n1, bs1, qs1, of1, ld1, lo1, 0);
		if (paired) take(b, (uint32_t)n2, bs2, qs2, of2, ld2, lo2, of1[n1]);
		if ((rc = b.d_bases.ensure(std::max<uint64_t>(nb, 1))) || (rc = b.d_offs.ensure(b.n + 1)) || (rc = b.d_verd.ensure(b.n))) break;
		if ((rc = hip_rc(hipMemcpyAsync(b.d_offs.p, b.offs.data(), (b.n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, B->st)))) break;
		if ((rc = hip_rc(hipMemcpyAsync(b.d_bases.p, b.h_bases, nb, hipMemcpyHostToDevice, B->st)))) break;
		if ((rc = urmapx_bitvec_search_device(B, b.d_bases.p, b.d_offs.p, b.n, b.d_verd.p))) break;
		if ((rc = hip_rc(hipMemcpyAsync(b.h_verd, b.d_verd.p, b.n, hipMemcpyDeviceToHost, B->st)))) break;
		if ((rc = hip_rc(hipEventRecord(b.done, B->st)))) break;
		b.busy = true;
		Batch &prev = bt[(k + 1) & 1];
		if (prev.busy && (rc = write_batch(prev))) break;  // while batch k is on the device
	}
	for (Batch &b : bt)  // the last batch (the loop above leaves at most one in flight)
		if (!rc && b.busy) rc = write_batch(b);
	for (Batch &b : bt)
		if (b.busy) (void)hipEventSynchronize(b.done);
	(void)urmapx_bitvec_sync(B);
	if (o1 && fclose(o1) != 0 && !rc) rc = URMAPX_E_IO;
	if (o2 && fclose(o2) != 0 && !rc) rc = URMAPX_E_IO;
	urmapx_fastq_close(F1);
	if (F2) urmapx_fastq_close(F2);
	if (counts) { counts[0] = found; counts[1] = total; }
	if (rc == URMAPX_E_IO && msg.empty()) msg = "write error";
	return rc ? fail(rc, msg.empty() ? urmapx_strerror(rc) : msg) : URMAPX_OK;
}
