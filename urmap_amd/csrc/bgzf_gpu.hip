// bgzf_gpu.hip -- SAM text resident in HBM -> BGZF members, deflated on the device (urmap -map / -map2 ... -bgzf).
//
// The text is cut every 65 280 bytes; one workgroup of 256 threads turns one piece into one complete gzip member
// (header with the 'BC' extra field, one deflate block, CRC-32, ISIZE):
//   crc      256 slices of the piece, one per thread, byte table in LDS; the slices' CRCs are folded pairwise with the
//            zero-extension operator (crc(A|B) = crc(A) * x^(8 |B|) mod P  xor  crc(B))
//   match    the piece is walked 256 positions at a time.  Every position of a step looks its 4-byte hash up in an LDS table of
//            4096 entries that holds positions of EARLIER steps only (entry = 1 + the largest position with that hash:
//            atomicMax, so the table does not depend on lane order), and tries distance 1 (runs).  The greedy parse of
//            the step -- which positions start a token -- is reachability from the step's entry position along
//            next[p] = p + (match ? length : 1): pointer doubling in LDS, 8 rounds.  Tokens go to a per-workgroup arena in
//            global memory in position order, their symbols into LDS histograms
//   codes    Huffman code lengths for the literal/length and the distance alphabet (rank sort by all threads, the two-queue
//            merge on one lane), limited to 15 bits; the code-length alphabet (zero runs as 17 / 18) limited to 7
//   bits     every thread sums the bit lengths of its run of tokens, a scan gives its first bit, it packs its tokens from
//            there.  Words shared by two threads are OR-ed (atomicOr into zeroed words: commutative, so deterministic)
//   stored   when the dynamic block would not be smaller than the piece + 5 bytes, the member holds a stored block
// A second kernel scans the members' sizes, a third moves them back to back into the caller's array.
#include "internal.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace urx;

namespace {

constexpr uint32_t PIECE = 65280;         // text bytes per member (htslib's BGZF_BLOCK_SIZE 0xff00)
constexpr uint32_t STRIDE = 65344;        // staging bytes per member: PIECE + 31 and room for the word behind the last one
constexpr uint32_t NT = 256;              // threads per workgroup
constexpr uint32_t HBITS = 12, HSIZE = 1u << HBITS;
constexpr uint32_t MAX_SLOTS = 1024;      // workgroups of a launch (each owns a token arena of PIECE words)
constexpr uint32_t NLL = 286, ND = 30, NCL = 19;
constexpr uint32_t HDR_WORDS = 192;       // member header + deflate block header as bits: 144 + 17 + 57 + 316 * 14 at most
constexpr uint32_t CRC_POLY = 0xedb88320u;

struct Lds {
	uint32_t table[HSIZE];
	uint32_t jmp[2][260];
	uint32_t mark[260];
	uint32_t cnt_ll[288], cnt_d[32], cnt_cl[32];
	uint32_t code_ll[288], code_d[32], code_cl[32];  // (length << 16) | bit-reversed code
	uint8_t len_ll[288], len_d[32], len_cl[32];
	// Huffman scratch
	uint16_t ord[288], leaf_par[288], node_par[288], node_depth[288];
	uint32_t sf[288], nf[288];
	uint32_t blc[16];
	uint32_t n_used;
	// code-length sequence: symbol | extra << 8
	uint16_t clseq[320];
	uint32_t n_clseq, hlit, hdist;
	uint32_t hdr[HDR_WORDS];
	uint32_t hdr_bits;
	uint32_t crc_tab[256];
	uint32_t x2n[32];
	uint32_t red[NT];
	uint32_t wave_cnt[4];
	uint32_t entry, crc;
};

__device__ __forceinline__ uint32_t load4(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint64_t load8(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

// a * b mod P, polynomials over GF(2) in the reflected representation (x^0 is bit 31)
__device__ uint32_t mulmodp(uint32_t a, uint32_t b) {
	uint32_t p = 0;
	for (uint32_t m = 0x80000000u; m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
	}
	return p;
}
// x^(8 n) mod P
__device__ uint32_t xpow8(const uint32_t *x2n, uint32_t n) {
	uint32_t p = 0x80000000u;
	for (uint32_t k = 3; n; n >>= 1, ++k)
		if (n & 1u) p = mulmodp(x2n[k], p);
	return p;
}

__device__ uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t maxl) {
	uint32_t l = 0;
	while (l + 8 <= maxl) {
		const uint64_t x = load8(a + l) ^ load8(b + l);
		if (x) return l + ((uint32_t)__builtin_ctzll(x) >> 3);
		l += 8;
	}
	while (l < maxl && a[l] == b[l]) ++l;
	return l;
}

__device__ __forceinline__ void len_symbol(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
	if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
	const uint32_t l = len - 3;
	if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
	eb = 29u - (uint32_t)__builtin_clz(l);
	sym = 261 + 4 * eb + ((l >> eb) & 3u);
	ev = l & ((1u << eb) - 1u);
}
__device__ __forceinline__ void dist_symbol(uint32_t d /* distance - 1 */, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
	if (d < 4) { sym = d; eb = 0; ev = 0; return; }
	const uint32_t lg = 31u - (uint32_t)__builtin_clz(d);
	eb = lg - 1;
	sym = 2 * lg + ((d >> eb) & 1u);
	ev = d & ((1u << eb) - 1u);
}

// Code lengths of at most maxbits for the n symbols counted in cnt, by the whole workgroup.  force2: an alphabet that may have fewer
// than two symbols in use gets its lowest unused ones counted once, so that the code is complete (the literal/length alphabet always
// has a literal and the end-of-block symbol).
__device__ void huff_lengths(Lds &S, uint32_t *cnt, uint32_t n, uint32_t maxbits, uint8_t *out, bool force2) {
	const uint32_t tid = threadIdx.x;
	if (tid == 0) {
		S.n_used = 0;
		for (uint32_t b = 0; b < 16; ++b) S.blc[b] = 0;
		if (force2) {
			uint32_t used = 0;
			for (uint32_t s = 0; s < n; ++s) used += cnt[s] != 0;
			for (uint32_t s = 0; s < n && used < 2; ++s)
				if (!cnt[s]) { cnt[s] = 1; ++used; }
		}
	}
	__syncthreads();
	for (uint32_t s = tid; s < n; s += NT) {
		out[s] = 0;
		const uint32_t c = cnt[s];
		if (!c) continue;
		uint32_t r = 0;
		for (uint32_t q = 0; q < n; ++q) {
			const uint32_t cq = cnt[q];
			r += (cq != 0) & ((cq < c) | ((cq == c) & (q < s)));
		}
		S.ord[r] = (uint16_t)s;
		S.sf[r] = c;
		atomicAdd(&S.n_used, 1u);
	}
	__syncthreads();
	const uint32_t m = S.n_used;
	if (tid == 0) {
		// leaves in rising order of count, internal nodes in the order they are made (rising too): the two smallest are at the two fronts
		uint32_t i = 0, j = 0;
		for (uint32_t k = 0; k + 1 < m; ++k) {
			uint32_t f = 0;
			for (int pick = 0; pick < 2; ++pick) {
				const bool leaf = i < m && (j >= k || S.sf[i] <= S.nf[j]);
				if (leaf) { f += S.sf[i]; S.leaf_par[i++] = (uint16_t)k; }
				else { f += S.nf[j]; S.node_par[j++] = (uint16_t)k; }
			}
			S.nf[k] = f;
		}
		S.node_depth[m - 2] = 0;
		for (uint32_t k = m - 2; k-- > 0;) S.node_depth[k] = (uint16_t)(S.node_depth[S.node_par[k]] + 1);
	}
	__syncthreads();
	for (uint32_t r = tid; r < m; r += NT) {
		uint32_t d = (uint32_t)S.node_depth[S.leaf_par[r]] + 1u;
		if (d > maxbits) d = maxbits;
		atomicAdd(&S.blc[d], 1u);
	}
	__syncthreads();
	if (tid == 0) {
		// lengths cut to maxbits oversubscribe the code by `over` units of 2^-maxbits; each step below takes one unit back: a leaf of the
		// deepest level above the last goes one down and one leaf of the last level comes up beside it
		uint32_t kraft = 0;
		for (uint32_t b = 1; b <= maxbits; ++b) kraft += S.blc[b] << (maxbits - b);
		for (uint32_t over = kraft > (1u << maxbits) ? kraft - (1u << maxbits) : 0u; over; --over) {
			uint32_t b = maxbits - 1;
			while (!S.blc[b]) --b;
			--S.blc[b]; S.blc[b + 1] += 2; --S.blc[maxbits];
		}
	}
	__syncthreads();
	// the rarest leaves get the longest codes
	for (uint32_t r = tid; r < m; r += NT) {
		uint32_t b = maxbits, cum = S.blc[maxbits];
		while (r >= cum) cum += S.blc[--b];
		out[S.ord[r]] = (uint8_t)b;
	}
	__syncthreads();
}

// canonical codes (RFC 1951 3.2.2), bit-reversed for an LSB-first stream; one thread
__device__ void assign_codes(const uint8_t *len, uint32_t n, uint32_t *code) {
	uint32_t blc[16], next[16];
	for (uint32_t b = 0; b < 16; ++b) blc[b] = 0;
	for (uint32_t s = 0; s < n; ++s) ++blc[len[s]];
	blc[0] = 0;
	uint32_t c = 0;
	next[0] = 0;
	for (uint32_t b = 1; b < 16; ++b) { c = (c + blc[b - 1]) << 1; next[b] = c; }
	for (uint32_t s = 0; s < n; ++s) {
		const uint32_t l = len[s];
		code[s] = l ? (l << 16) | (__brev(next[l]++) >> (32 - l)) : 0u;
	}
}

struct HdrBits {
	uint32_t *w;
	uint32_t n = 0;
	__device__ void put(uint32_t v, uint32_t nb) {
		const uint32_t i = n >> 5, sh = n & 31u;
		w[i] |= v << sh;
		if (sh + nb > 32) w[i + 1] |= v >> (32 - sh);
		n += nb;
	}
};

// a thread's part of the member's bit stream: whole words of its own are stored, the words it shares are OR-ed into zeroed memory
struct BitOut {
	uint32_t *words;
	uint64_t acc = 0;
	uint32_t fill, w;
	bool first_shared;
	__device__ BitOut(uint32_t *words_, uint32_t start_bit) : words(words_), fill(start_bit & 31u), w(start_bit >> 5), first_shared((start_bit & 31u) != 0) {}
	__device__ __forceinline__ void put(uint32_t v, uint32_t nb) {
		acc |= (uint64_t)v << fill;
		fill += nb;
		if (fill >= 32) {
			if (first_shared) { atomicOr(&words[w], (uint32_t)acc); first_shared = false; }
			else words[w] = (uint32_t)acc;
			acc >>= 32; fill -= 32; ++w;
		}
	}
	__device__ void finish() {
		if (fill) atomicOr(&words[w], (uint32_t)acc);
	}
};

__device__ __forceinline__ uint32_t token_bits(const Lds &S, uint32_t t) {
	const uint32_t len = t >> 16;
	if (!len) return S.code_ll[t] >> 16;
	uint32_t ls, leb, lev, ds, deb, dev;
	len_symbol(len, ls, leb, lev);
	dist_symbol(t & 0xffffu, ds, deb, dev);
	return (S.code_ll[ls] >> 16) + leb + (S.code_d[ds] >> 16) + deb;
}

__global__ __launch_bounds__(NT) void bgzf_piece_kernel(const uint8_t *text, uint64_t n_total, uint32_t n_pieces, uint8_t *stage, uint32_t *tokens,
                                                         uint32_t *sizes) {
	__shared__ Lds S;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	uint32_t *tok = tokens + (size_t)blockIdx.x * PIECE;
	// tables that do not depend on the piece
	{
		uint32_t c = tid;
		for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
		S.crc_tab[tid] = c;
		if (tid == 0) {
			uint32_t p = 0x40000000u;  // x^1
			S.x2n[0] = p;
			for (int k = 1; k < 32; ++k) S.x2n[k] = p = mulmodp(p, p);
		}
	}
	__syncthreads();
	for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
		const uint8_t *in = text + (size_t)piece * PIECE;
		const uint64_t left = n_total - (uint64_t)piece * PIECE;
		const uint32_t n = left < PIECE ? (uint32_t)left : PIECE;  // >= 1
		uint8_t *out = stage + (size_t)piece * STRIDE;
		uint32_t *outw = (uint32_t *)out;

		// ---- CRC-32 ----
		const uint32_t slice = (n + NT - 1) / NT;
		{
			const uint32_t lo = min(tid * slice, n), hi = min(lo + slice, n);
			uint32_t c = 0xffffffffu;
			for (uint32_t i = lo; i < hi; ++i) c = S.crc_tab[(c ^ in[i]) & 0xffu] ^ (c >> 8);
			S.red[tid] = hi > lo ? ~c : 0u;  // (the CRC of nothing is 0)
		}
		for (uint32_t i = tid; i < HSIZE; i += NT) S.table[i] = 0;
		for (uint32_t i = tid; i < 288; i += NT) S.cnt_ll[i] = 0;
		if (tid < 32) { S.cnt_d[tid] = 0; S.cnt_cl[tid] = 0; }
		if (tid == 0) S.entry = 0;
		__syncthreads();
		for (uint32_t w = 1; w < NT; w <<= 1) {  // slices [tid, tid + w) and [tid + w, tid + 2w) become one
			if ((tid & (2 * w - 1)) == 0) {
				const uint32_t b0 = min((tid + w) * slice, n), b1 = min((tid + 2 * w) * slice, n);
				S.red[tid] = mulmodp(xpow8(S.x2n, b1 - b0), S.red[tid]) ^ S.red[tid + w];
			}
			__syncthreads();
		}
		if (tid == 0) S.crc = S.red[0];

		// ---- matches, greedy parse, tokens ----
		uint32_t ntok = 0;
		for (uint32_t base = 0; base < n; base += NT) {
			const uint32_t p = base + tid;
			const uint32_t entry = S.entry;
			const bool hashed = p + 4 <= n;
			uint32_t h = 0;
			if (hashed) h = (load4(in + p) * 2654435761u) >> (32 - HBITS);
			const bool parse = entry < base + NT;  // uniform
			uint32_t best_len = 0, best_dist = 0;
			if (parse && p >= entry && p < n) {
				const uint32_t maxl = min(258u, n - p);
				if (hashed) {
					const uint32_t c = S.table[h];
					if (c && p - (c - 1) <= 32768u) {
						const uint32_t l = match_len(in + (c - 1), in + p, maxl);
						// (a short match far away costs more bits than its literals: zlib's TOO_FAR rule, here for lengths 4 and 5)
					if (l >= 6 || (l >= 4 && p - (c - 1) <= 4096u)) { best_len = l; best_dist = p - (c - 1); }
					}
				}
				if (p >= 1 && maxl >= 3) {
					const uint32_t l = match_len(in + p - 1, in + p, maxl);
					if (l >= 3 && l >= best_len) { best_len = l; best_dist = 1; }
				}
			}
			const uint32_t step = best_len ? best_len : 1u;
			if (parse) {
				S.jmp[0][tid] = (p + step >= n) ? 256u : min(tid + step, 256u);
				S.mark[tid] = p == entry ? 1u : 0u;
				if (tid == 0) { S.jmp[0][256] = 256; S.jmp[1][256] = 256; S.mark[256] = 0; }
			}
			__syncthreads();  // every look-up of the step is behind this: the step's own positions go into the table now
			if (hashed) atomicMax(&S.table[h], p + 1);
			if (!parse) { __syncthreads(); continue; }  // (a match reaches over the whole step: its positions are only entered)
			for (int k = 0; k < 8; ++k) {
				const uint32_t *src = S.jmp[k & 1];
				uint32_t *dst = S.jmp[(k & 1) ^ 1];
				const uint32_t j = src[tid];
				// marks only ever appear, and only on positions the parse reaches: a mark seen early changes nothing.  Threads read and set
				// them within one round, so both sides are relaxed atomics
				if (__hip_atomic_load(&S.mark[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
					__hip_atomic_store(&S.mark[j], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
				dst[tid] = src[j];
				__syncthreads();
			}
			const bool mine = S.mark[tid] != 0 && p < n;
			const uint64_t bal = __ballot(mine);
			if (lane == 0) S.wave_cnt[wave] = (uint32_t)__popcll(bal);
			if (mine && p + step >= base + NT) S.entry = p + step;  // one thread: the step's last token
			__syncthreads();
			uint32_t before = 0, total = 0;
			for (uint32_t w = 0; w < 4; ++w) { const uint32_t c = S.wave_cnt[w]; total += c; if (w < wave) before += c; }
			if (mine) {
				const uint32_t at = ntok + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
				if (best_len) {
					uint32_t s, eb, ev;
					tok[at] = (best_len << 16) | (best_dist - 1);
					len_symbol(best_len, s, eb, ev);
					atomicAdd(&S.cnt_ll[s], 1u);
					dist_symbol(best_dist - 1, s, eb, ev);
					atomicAdd(&S.cnt_d[s], 1u);
				} else {
					const uint32_t b = in[p];
					tok[at] = b;
					atomicAdd(&S.cnt_ll[b], 1u);
				}
			}
			ntok += total;
			__syncthreads();  // (wave_cnt, mark and jmp are the next step's)
		}
		if (tid == 0) S.cnt_ll[256] = 1;
		__syncthreads();

		// ---- codes ----
		huff_lengths(S, S.cnt_ll, NLL, 15, S.len_ll, false);
		huff_lengths(S, S.cnt_d, ND, 15, S.len_d, true);
		if (tid == 0) {
			uint32_t hlit = NLL, hdist = ND;
			while (hlit > 257 && !S.len_ll[hlit - 1]) --hlit;
			while (hdist > 1 && !S.len_d[hdist - 1]) --hdist;
			S.hlit = hlit; S.hdist = hdist;
			// the two alphabets' lengths as one sequence; runs of zeros as 17 (3..10) and 18 (11..138)
			const uint32_t tot = hlit + hdist;
			uint32_t k = 0, i = 0;
			while (i < tot) {
				const uint32_t l = i < hlit ? S.len_ll[i] : S.len_d[i - hlit];
				uint32_t run = 1;
				if (l == 0)
					while (i + run < tot && run < 138 && (i + run < hlit ? S.len_ll[i + run] : S.len_d[i + run - hlit]) == 0) ++run;
				uint32_t sym = l, ext = 0;
				if (l == 0 && run >= 11) { sym = 18; ext = run - 11; }
				else if (l == 0 && run >= 3) { sym = 17; ext = run - 3; }
				else run = 1;
				S.clseq[k++] = (uint16_t)(sym | (ext << 8));
				++S.cnt_cl[sym];
				i += run;
			}
			S.n_clseq = k;
		}
		__syncthreads();
		huff_lengths(S, S.cnt_cl, NCL, 7, S.len_cl, true);
		if (tid == 0) assign_codes(S.len_ll, NLL, S.code_ll);
		if (tid == 64) assign_codes(S.len_d, ND, S.code_d);
		if (tid == 128) assign_codes(S.len_cl, NCL, S.code_cl);
		for (uint32_t i = tid; i < HDR_WORDS; i += NT) S.hdr[i] = 0;
		__syncthreads();
		if (tid == 0) {
			HdrBits H{S.hdr};
			H.put(0x04088b1fu, 32);  // ID1 ID2 CM=8 FLG=FEXTRA
			H.put(0, 32);            // MTIME
			H.put(0xff00u, 16);      // XFL, OS = unknown
			H.put(6, 16);            // XLEN
			H.put(0x00024342u, 32);  // 'B' 'C', subfield length 2
			H.put(0, 16);            // BSIZE: set when the size is known
			H.put(1, 1); H.put(2, 2);  // BFINAL, BTYPE = dynamic
			const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
			uint32_t hclen = 19;
			while (hclen > 4 && !S.len_cl[order[hclen - 1]]) --hclen;
			H.put(S.hlit - 257, 5); H.put(S.hdist - 1, 5); H.put(hclen - 4, 4);
			for (uint32_t i = 0; i < hclen; ++i) H.put(S.len_cl[order[i]], 3);
			for (uint32_t i = 0; i < S.n_clseq; ++i) {
				const uint32_t sym = S.clseq[i] & 0xffu, ext = S.clseq[i] >> 8, c = S.code_cl[sym];
				H.put(c & 0xffffu, c >> 16);
				if (sym == 17) H.put(ext, 3);
				else if (sym == 18) H.put(ext, 7);
			}
			S.hdr_bits = H.n;
		}
		__syncthreads();

		// ---- bit lengths, their prefix sum ----
		const uint32_t per = (ntok + NT - 1) / NT;
		const uint32_t t0 = min(tid * per, ntok), t1 = min(t0 + per, ntok);
		uint32_t my_bits = 0;
		for (uint32_t i = t0; i < t1; ++i) my_bits += token_bits(S, tok[i]);
		if (tid == 0) my_bits += S.hdr_bits;
		if (tid == NT - 1) my_bits += S.code_ll[256] >> 16;
		S.red[tid] = my_bits;
		__syncthreads();
		for (uint32_t w = 1; w < NT; w <<= 1) {
			const uint32_t v = tid >= w ? S.red[tid - w] : 0u;
			__syncthreads();
			S.red[tid] += v;
			__syncthreads();
		}
		const uint32_t end_bit = S.red[tid], start_bit = end_bit - my_bits;
		const uint32_t deflate_end = (S.red[NT - 1] + 7) >> 3;  // bytes of the member up to the end of the deflate block
		const uint32_t crc = S.crc;
		uint32_t member;
		if (deflate_end + 8 < n + 31) {
			member = deflate_end + 8;
			const uint32_t last_end = (member << 3);
			outw[start_bit >> 5] = 0;
			outw[(tid == NT - 1 ? last_end : end_bit) >> 5] = 0;
			if (tid == 0) S.hdr[4] |= (member - 1) << 0;  // BSIZE: bytes 16..17
			__syncthreads();
			BitOut B(outw, start_bit);
			if (tid == 0) {
				const uint32_t hb = S.hdr_bits;
				for (uint32_t i = 0; i < (hb >> 5); ++i) B.put(S.hdr[i], 32);
				if (hb & 31u) B.put(S.hdr[hb >> 5], hb & 31u);
			}
			for (uint32_t i = t0; i < t1; ++i) {
				const uint32_t t = tok[i], len = t >> 16;
				if (!len) { const uint32_t c = S.code_ll[t]; B.put(c & 0xffffu, c >> 16); continue; }
				uint32_t ls, leb, lev, ds, deb, dev;
				len_symbol(len, ls, leb, lev);
				dist_symbol(t & 0xffffu, ds, deb, dev);
				const uint32_t cl = S.code_ll[ls], cd = S.code_d[ds];
				B.put((cl & 0xffffu) | (lev << (cl >> 16)), (cl >> 16) + leb);
				B.put((cd & 0xffffu) | (dev << (cd >> 16)), (cd >> 16) + deb);
			}
			if (tid == NT - 1) {
				const uint32_t c = S.code_ll[256];
				B.put(c & 0xffffu, c >> 16);
				const uint32_t pad = (deflate_end << 3) - end_bit;
				if (pad) B.put(0, pad);
				B.put(crc, 32);
				B.put(n, 32);
			}
			B.finish();
		} else {
			// stored: 18 bytes of header, BFINAL + BTYPE 0 in a byte of their own, LEN, NLEN, the text, CRC-32, ISIZE
			member = n + 31;
			if (tid < 31) {
				const uint32_t bs = member - 1, nl = ~n;
				const uint8_t head[23] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bs, (uint8_t)(bs >> 8),
				                          1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)nl, (uint8_t)(nl >> 8)};
				if (tid < 23) out[tid] = head[tid];
				else if (tid < 27) out[n + tid] = (uint8_t)(crc >> (8 * (tid - 23)));
				else out[n + tid] = (uint8_t)(n >> (8 * (tid - 27)));
			}
			for (uint32_t i = tid; i < n; i += NT) out[23 + i] = in[i];
		}
		if (tid == 0) sizes[piece] = member;
		__syncthreads();
	}
}

// huff_lengths alone (urmapx_bgzf_code_lengths): one workgroup, counts[n] through the literal/length histogram of the piece kernel's LDS
__global__ __launch_bounds__(NT) void bgzf_code_lengths_kernel(const uint32_t *counts, uint32_t n, uint32_t maxbits, int force2, uint8_t *out) {
	__shared__ Lds S;
	for (uint32_t s = threadIdx.x; s < n; s += NT) S.cnt_ll[s] = counts[s];
	__syncthreads();
	huff_lengths(S, S.cnt_ll, n, maxbits, S.len_ll, force2 != 0);
	for (uint32_t s = threadIdx.x; s < n; s += NT) out[s] = S.len_ll[s];
}

// exclusive prefix sum of the members' sizes; the end-of-file member and the total
__global__ __launch_bounds__(1024) void bgzf_scan_kernel(const uint32_t *sizes, uint32_t n_pieces, uint64_t *offs, uint8_t *out, int with_eof, uint64_t *used) {
	__shared__ uint64_t part[1024];
	__shared__ uint64_t carry;
	const uint32_t tid = threadIdx.x;
	if (tid == 0) carry = 0;
	__syncthreads();
	for (uint32_t base = 0; base < n_pieces; base += 1024) {
		const uint32_t i = base + tid;
		const uint64_t v = i < n_pieces ? sizes[i] : 0;
		part[tid] = v;
		__syncthreads();
		for (uint32_t w = 1; w < 1024; w <<= 1) {
			const uint64_t a = tid >= w ? part[tid - w] : 0;
			__syncthreads();
			part[tid] += a;
			__syncthreads();
		}
		if (i < n_pieces) offs[i] = carry + part[tid] - v;
		__syncthreads();
		if (tid == 1023) carry += part[1023];
		__syncthreads();
	}
	if (tid < 28 && with_eof) {
		const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		out[carry + tid] = eof[tid];
	}
	if (tid == 0) *used = carry + (with_eof ? 28u : 0u);
}

// member i from its staging slot to offs[i] of the output
__global__ __launch_bounds__(NT) void bgzf_pack_kernel(const uint8_t *stage, const uint32_t *sizes, const uint64_t *offs, uint32_t n_pieces, uint8_t *out) {
	for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
		const uint8_t *src = stage + (size_t)piece * STRIDE;
		uint8_t *dst = out + offs[piece];
		const uint32_t n = sizes[piece];
		const uint32_t head = min(n, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
		if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
		const uint32_t words = (n - head) >> 2;
		uint32_t *dw = (uint32_t *)(dst + head);
		for (uint32_t i = threadIdx.x; i < words; i += NT) dw[i] = load4(src + head + 4 * i);
		const uint32_t done = head + 4 * words;
		if (threadIdx.x < n - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
	}
}

}  // namespace

struct urmapx_bgzf {
	int device = 0;
	hipStream_t st = nullptr;
	DevBuf<uint8_t> stage;
	DevBuf<uint32_t> tokens, sizes;
	DevBuf<uint64_t> offs;
};

extern "C" {

int urmapx_bgzf_create(int device, void *stream, urmapx_bgzf **out) {
	if (!out) return URMAPX_E_ARG;
	*out = nullptr;
	HIP_TRY(hipSetDevice(device));
	urmapx_bgzf *Z = new urmapx_bgzf;
	Z->device = device;
	Z->st = (hipStream_t)stream;
	*out = Z;
	return URMAPX_OK;
}

void urmapx_bgzf_destroy(urmapx_bgzf *Z) {
	if (!Z) return;
	(void)hipSetDevice(Z->device);
	(void)hipStreamSynchronize(Z->st);
	Z->stage.release(); Z->tokens.release(); Z->sizes.release(); Z->offs.release();
	delete Z;
}

// workgroups of a piece launch at most: MAX_SLOTS, or fewer under the test aid URMAPX_TEST_BGZF_SLOTS=N (1..MAX_SLOTS), which makes
// a workgroup take a second piece on a small input.  The arenas are sized by it and the launch's grid is it: one value for both
static uint32_t bgzf_slots() {
	static const uint32_t slots = [] {
		const char *e = getenv("URMAPX_TEST_BGZF_SLOTS");
		const long v = e ? atol(e) : 0;
		return v >= 1 && v < (long)MAX_SLOTS ? (uint32_t)v : MAX_SLOTS;
	}();
	return slots;
}

// the launches' scratch for n bytes of text; a no-op once it is large enough
static int bgzf_reserve(urmapx_bgzf *Z, size_t n) {
	const uint32_t n_pieces = (uint32_t)((n + PIECE - 1) / PIECE);
	const uint32_t grid = n_pieces < bgzf_slots() ? n_pieces : bgzf_slots();
	int rc;
	// (a growing array is replaced: what the stream still reads from the old one has to be over)
	if (Z->stage.cap < (size_t)n_pieces * STRIDE || Z->tokens.cap < (size_t)grid * PIECE || Z->sizes.cap < n_pieces + 1u || Z->offs.cap < n_pieces + 1u)
		HIP_TRY(hipStreamSynchronize(Z->st));
	if ((rc = Z->stage.ensure((size_t)n_pieces * STRIDE))) return rc;
	if ((rc = Z->tokens.ensure((size_t)grid * PIECE))) return rc;
	if ((rc = Z->sizes.ensure(n_pieces + 1u))) return rc;
	if ((rc = Z->offs.ensure(n_pieces + 1u))) return rc;
	return URMAPX_OK;
}

int urmapx_bgzf_compress_device(int device, const void *d_in, size_t n, void *d_out, size_t out_cap, uint64_t *d_used, int with_eof, urmapx_bgzf *Z) {
	if (!Z || Z->device != device || !d_out || !d_used || (n && !d_in)) return URMAPX_E_ARG;
	if (out_cap < urmapx_bgzf_bound(n) || n > ((size_t)1 << 36)) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(device));
	const uint32_t n_pieces = (uint32_t)((n + PIECE - 1) / PIECE);
	const uint32_t grid = n_pieces < bgzf_slots() ? n_pieces : bgzf_slots();
	int rc;
	if ((rc = bgzf_reserve(Z, n))) return rc;
	if (n_pieces) {
		hipLaunchKernelGGL(bgzf_piece_kernel, dim3(grid), dim3(NT), 0, Z->st, (const uint8_t *)d_in, (uint64_t)n, n_pieces, Z->stage.p, Z->tokens.p, Z->sizes.p);
	}
	hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(1024), 0, Z->st, Z->sizes.p, n_pieces, Z->offs.p, (uint8_t *)d_out, with_eof, d_used);
	if (n_pieces) {
		const uint32_t pg = n_pieces < 4096u ? n_pieces : 4096u;
		hipLaunchKernelGGL(bgzf_pack_kernel, dim3(pg), dim3(NT), 0, Z->st, Z->stage.p, Z->sizes.p, Z->offs.p, n_pieces, (uint8_t *)d_out);
	}
	HIP_TRY(hipGetLastError());
	return URMAPX_OK;
}

int urmapx_bgzf_compress_timed(int device, const void *in, size_t n, void *out, size_t cap, size_t *used, int with_eof, float *ms) {
	if (!out || !used || (n && !in)) return URMAPX_E_ARG;
	if (cap < urmapx_bgzf_bound(n)) return URMAPX_E_ARG;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	HIP_TRY(hipSetDevice(device));
	urmapx_bgzf *Z = nullptr;
	int rc = urmapx_bgzf_create(device, nullptr, &Z);
	if (rc) return rc;
	DevBuf<uint8_t> d_in, d_out;
	DevBuf<uint64_t> d_used;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	uint64_t got = 0;
	const size_t bound = urmapx_bgzf_bound(n);
	auto run = [&]() -> int {
		int r;
		if ((r = d_in.ensure(n + 16))) return r;
		if ((r = d_out.ensure(bound + 16))) return r;
		if ((r = d_used.ensure(1))) return r;
		if (n) HIP_TRY(hipMemcpy(d_in.p, in, n, hipMemcpyHostToDevice));
		if ((r = bgzf_reserve(Z, n))) return r;  // (before the first event: *ms is the three launches, no allocation call among them)
		HIP_TRY(hipEventCreate(&e0));
		HIP_TRY(hipEventCreate(&e1));
		HIP_TRY(hipEventRecord(e0, nullptr));
		if ((r = urmapx_bgzf_compress_device(device, d_in.p, n, d_out.p, bound, d_used.p, with_eof, Z))) return r;
		HIP_TRY(hipEventRecord(e1, nullptr));
		HIP_TRY(hipMemcpy(&got, d_used.p, 8, hipMemcpyDeviceToHost));
		if (got > cap) return URMAPX_E_ARG;
		if (got) HIP_TRY(hipMemcpy(out, d_out.p, got, hipMemcpyDeviceToHost));
		if (ms) { *ms = 0; (void)hipEventElapsedTime(ms, e0, e1); }
		return URMAPX_OK;
	};
	rc = run();
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	urmapx_bgzf_destroy(Z);
	d_in.release(); d_out.release(); d_used.release();
	if (!rc) *used = (size_t)got;
	return rc;
}

int urmapx_bgzf_compress(int device, const void *in, size_t n, void *out, size_t cap, size_t *used, int with_eof) {
	return urmapx_bgzf_compress_timed(device, in, n, out, cap, used, with_eof, nullptr);
}

int urmapx_bgzf_code_lengths(int device, const uint32_t *counts, uint32_t n, uint32_t maxbits, int force2, uint8_t *lengths) {
	if (!counts || !lengths || n < 2 || n > NLL || maxbits < 1 || maxbits > 15) return URMAPX_E_ARG;
	// what huff_lengths relies on: two symbols in use at least (its tree has used - 1 >= 1 nodes), a code of maxbits bits that can hold
	// them, node weights that fit 32 bits
	uint32_t used = 0;
	uint64_t sum = 0;
	for (uint32_t s = 0; s < n; ++s) { used += counts[s] != 0; sum += counts[s]; }
	if (force2 && used < 2) { sum += 2 - used; used = 2; }
	if (used < 2 || used > (1u << maxbits) || sum > 0xffffffffull) return URMAPX_E_ARG;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	HIP_TRY(hipSetDevice(device));
	DevBuf<uint32_t> d_cnt;
	DevBuf<uint8_t> d_len;
	auto run = [&]() -> int {
		int r;
		if ((r = d_cnt.ensure(n))) return r;
		if ((r = d_len.ensure(n))) return r;
		HIP_TRY(hipMemcpy(d_cnt.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice));
		hipLaunchKernelGGL(bgzf_code_lengths_kernel, dim3(1), dim3(NT), 0, nullptr, d_cnt.p, n, maxbits, force2, d_len.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(lengths, d_len.p, n, hipMemcpyDeviceToHost));
		return URMAPX_OK;
	};
	const int rc = run();
	d_cnt.release(); d_len.release();
	return rc;
}

}  // extern "C"
