// bam_gpu.hip -- the BAM alignment records of a chunk, encoded on the device (urmapx_text_set_bam; include/urmapx.h "BAM output").
//
// The text stage (text_gpu.hip) runs these two kernels where it runs sam_len_kernel and sam_kernel for SAM text; everything around
// them -- the parse, the mapping, the prefix sum of the record lengths, the BGZF compressor behind them, the copy back -- is the same.
// A record holds what the SAM record of the same read holds (SetSAM / SetSAM2, setsam.cpp, output2.cpp), in the layout of SAM/BAM
// specification v1 section 4.2:
//
//   block_size refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen    36 bytes, nine words
//   read_name\0   cigar[n_cigar_op] (len << 4 | op)   seq[(l_seq + 1) / 2] (4 bits a base)   qual[l_seq] (Phred, no + 33)
//
//   bam_len_kernel   one THREAD per record: its length (nothing is written but a number), the HitStats counters
//   bam_kernel       64 records per wavefront at a time: every LANE builds the nine core words and the CIGAR words of its own
//                    record in its slice of LDS, then the wavefront goes through its 64 records and writes core, name, CIGAR, the
//                    packed bases and the qualities with all lanes
#include "internal.h"
#include "text_dev.h"

namespace {

constexpr int GRID = 2048;
constexpr int BAM_CORE_WORDS = 9;
constexpr int BAM_SMALL_OPS = 15;   // CIGAR words a lane's LDS slice takes: core + these = 96 bytes; a longer CIGAR goes straight to the output
constexpr int BAM_SLICE = 25;       // words from one lane's slice to the next: 24 used, odd so that the 64 lanes' stores fall into 64 banks
constexpr uint32_t BAM_MAX_QNAME = 254, BAM_MAX_CIGAR = 65535;

// section 5.3 (beg >= 0 here: an unplaced record's bin is the constant 4680)
__device__ __forceinline__ uint32_t reg2bin(uint32_t beg, uint32_t end) {
	--end;
	if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
	if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
	if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
	if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
	if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
	return 0u;
}

// the flags SetSAM_Unmapped keeps of the ones it is given (setsam.cpp:14-27)
__device__ __forceinline__ uint32_t unmapped_flags(uint32_t given) {
	uint32_t flags = 0x04u;
	if (given & 0x01u) flags |= 0x01u;
	if (given & 0x40u) flags |= 0x40u;
	else if (given & 0x80u) flags |= 0x80u;
	if (given & 0x08u) flags |= 0x08u;
	else if (given & 0x20u) flags |= 0x20u;
	return flags;
}

// CIGAR ops of a record: none for an unmapped read, one ("<QL>M") without a path, else the merged runs less the dangling M
__device__ uint32_t cigar_op_count(const SamArgs &A, const urmapx_result &r) {
	if (r.dbpos == 0xFFFFFFFFu) return 0u;
	if (r.path_nops == 0) return 1u;
	CigarEnds E;
	cigar_ends(A.ops + r.path_off, r.path_nops, E);
	if (E.N >= 3) {
		if (E.fo[0] == 'M' && E.fl[0] <= 2 && E.fl[1] > 4 && E.fo[2] == 'M') return E.N - 1u;
		if (E.lo[2] == 'M' && E.ll[2] <= 2 && E.ll[1] > 4 && E.lo[0] == 'M') return E.N - 1u;
	}
	return E.N;
}

__device__ __forceinline__ uint32_t record_bytes(uint32_t qn, uint32_t n_cigar, uint32_t QL) {  // block_size and the field itself
	return 4u * BAM_CORE_WORDS + qn + 1u + 4u * n_cigar + (QL + 1u) / 2u + QL;
}

// QNAME of a record's label line: "/1" "/2" dropped, cut at the first blank (setsam.cpp:36-46), as sam_len_kernel has it
__device__ __forceinline__ uint32_t qname_bytes(const uint8_t *label, uint32_t ln) {
	if (ln > 2 && label[ln - 2] == '/' && (label[ln - 1] == '1' || label[ln - 1] == '2')) ln -= 2;
	uint32_t qn = 0;
	while (qn < ln && label[qn] != ' ' && label[qn] != '\t') ++qn;
	return qn;
}

// PASS 0: record lengths and the HitStats counters (output1.cpp:20-30), one thread per record.  Flag 8 (the chunk is handed back to
// the host road, which says why): a QNAME that does not fit l_read_name, a sequence index outside the index.
__global__ __launch_bounds__(256) void bam_len_kernel(SamArgs A) {
	const uint32_t n = A.hdr->n_reads;
	uint32_t c_acc = 0, c_rej = 0, c_no = 0, c_uns = 0;
	bool bad = false;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const urmapx_result r = A.results[i];
		const RecView V = record_view(A, i, r);
		const uint32_t qn = qname_bytes(V.raw + V.s1 + 1u, V.e1 - V.s1 - 1u);
		const uint32_t nc = cigar_op_count(A, r);
		A.lens[i] = record_bytes(qn, nc, V.QL);
		A.qn[i] = qn;
		if (qn > BAM_MAX_QNAME || nc > BAM_MAX_CIGAR) bad = true;
		if (r.dbpos != 0xFFFFFFFFu && (r.seq_index >= A.seq_count || (V.F.mate_mapped && V.F.mate_seq_index >= A.seq_count))) bad = true;
		if (r.status) ++c_uns;
		if (r.dbpos == 0xFFFFFFFFu) ++c_no;
		else if (r.mapq >= A.minq) ++c_acc;
		else ++c_rej;
	}
	if (bad) atomicOr(&A.hdr->flags, 8u);
	for (int d = 32; d; d >>= 1) {
		c_acc += __shfl_xor(c_acc, d, 64); c_rej += __shfl_xor(c_rej, d, 64);
		c_no += __shfl_xor(c_no, d, 64); c_uns += __shfl_xor(c_uns, d, 64);
	}
	__shared__ uint32_t s_cnt[4];  // one atomic per block and counter on the launch's four addresses, as in sam_len_kernel
	if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	if ((threadIdx.x & 63) == 0) {
		if (c_acc) atomicAdd(&s_cnt[0], c_acc);
		if (c_rej) atomicAdd(&s_cnt[1], c_rej);
		if (c_no) atomicAdd(&s_cnt[2], c_no);
		if (c_uns) atomicAdd(&s_cnt[3], c_uns);
	}
	__syncthreads();
	if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&A.hdr->cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// Where a lane puts the words of its record: word 0..8 the core, 9.. the CIGAR.  `cap` words were reserved; one more is not stored
// (and the count that comes back gives the record away).
struct WordsLds {
	lds_ptr<uint32_t> base;
	uint32_t cap;
	__device__ __forceinline__ void put(uint32_t i, uint32_t v) { if (i < cap) base[i] = v; }
};
struct WordsGlobal {  // a CIGAR longer than the slice: straight into the record, byte by byte (a record starts at any address)
	uint8_t *rec;
	uint32_t cigar_at, cap;
	__device__ __forceinline__ void put(uint32_t i, uint32_t v) {
		if (i >= cap) return;
		uint8_t *p = rec + (i < (uint32_t)BAM_CORE_WORDS ? 4u * i : cigar_at + 4u * (i - BAM_CORE_WORDS));
		p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
	}
};

// The core and the CIGAR of one record; returns n_cigar_op, or UINT32_MAX for a record the encoder does not take.
template <class W>
__device__ uint32_t build_words(const SamArgs &A, const urmapx_result &r, const MateFields &F, uint32_t QL, uint32_t qn, W &w) {
	uint32_t ref_id = 0xFFFFFFFFu, pos = 0xFFFFFFFFu, next_id = 0xFFFFFFFFu, next_pos = 0xFFFFFFFFu;
	uint32_t mapq = 0, bin = 4680u, nc = 0, flags, tlen = 0;
	if (r.dbpos == 0xFFFFFFFFu) flags = unmapped_flags(F.flags);
	else {
		flags = F.flags;
		if (r.seq_index >= A.seq_count) return 0xFFFFFFFFu;
		ref_id = r.seq_index; pos = r.coord; mapq = r.mapq; tlen = (uint32_t)F.tlen;
		uint32_t span = 0;  // reference bases under the CIGAR: M and D
		if (r.path_nops == 0) { w.put(BAM_CORE_WORDS, QL << 4); nc = 1; span = QL; }
		else {
			const urmapx_path_op *ops = A.ops + r.path_off;
			CigarEnds E;
			cigar_ends(ops, r.path_nops, E);
			walk_cigar_runs(ops, r.path_nops, E, [&](uint32_t len, char op) {
				w.put(BAM_CORE_WORDS + nc, len << 4 | (op == 'M' ? 0u : op == 'I' ? 1u : 2u));
				++nc;
				if (op != 'I') span += len;
			});
		}
		bin = reg2bin(pos, pos + (span ? span : 1u));
		// RNEXT as build_head prints it: '*' without a mapped mate or for a target without a name, '=' (refID) for the same label
		if (F.mate_mapped) {
			if (F.mate_seq_index >= A.seq_count) return 0xFFFFFFFFu;
			const uint32_t t0 = A.tname_offs[r.seq_index], tl = A.tname_offs[r.seq_index + 1] - t0;
			const uint32_t m0 = A.tname_offs[F.mate_seq_index], ml = A.tname_offs[F.mate_seq_index + 1] - m0;
			bool same = ml == tl;
			if (F.mate_seq_index != r.seq_index)
				for (uint32_t i = 0; same && i < tl; ++i) same = A.tnames[t0 + i] == A.tnames[m0 + i];
			if (ml == 0 || (ml == 1 && A.tnames[m0] == '*')) next_id = 0xFFFFFFFFu;
			else next_id = same ? ref_id : F.mate_seq_index;
			if (F.mate_coord != 0 && F.mate_coord != 0xFFFFFFFFu) next_pos = F.mate_coord;  // (position 0 prints as 0: setsam.cpp:168-172)
		}
	}
	w.put(0, record_bytes(qn, nc, QL) - 4u);
	w.put(1, ref_id);
	w.put(2, pos);
	w.put(3, (qn + 1u) | mapq << 8 | bin << 16);
	w.put(4, nc | flags << 16);
	w.put(5, QL);
	w.put(6, next_id);
	w.put(7, next_pos);
	w.put(8, tlen);
	return nc;
}

// PASS 1.  A record's length must be the one bam_len_kernel reserved; if not, the chunk is flagged and handed back (flag 32).
// Two bases share a byte and a lane owns whole bytes: lane j of a round packs bases 2j and 2j + 1 (from the far end of the read for a
// minus-strand hit, complemented), so no byte is written twice.
__global__ __launch_bounds__(SAM_WAVES * 64) void bam_kernel(SamArgs A) {
	__shared__ uint32_t s_words[SAM_WAVES][64 * BAM_SLICE];
	__shared__ uint8_t s_nib[2][256];  // [0] letter -> code, [1] letter -> code of its complement
	s_nib[0][threadIdx.x] = (uint8_t)nibble_of(threadIdx.x);
	s_nib[1][threadIdx.x] = (uint8_t)nibble_of(A.comp[threadIdx.x]);
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t n = A.hdr->n_reads;
	const uint32_t wave = blockIdx.x * SAM_WAVES + w, n_waves = gridDim.x * SAM_WAVES;
	uint8_t *const dst = (uint8_t *)A.sam;
	for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
		const uint32_t i = base + (uint32_t)lane;
		uint32_t qn = 0, off = 0, nc = 0, QL = 0, s1 = 0, e1 = 0, e3 = 0, fl = 0;  // fl: 1 words in LDS, 2 bad, 4 plus, 8 words already in the record
		if (i < n) {
			const urmapx_result r = A.results[i];
			const RecView V = record_view(A, i, r);
			qn = A.qn[i]; off = A.rec_offs[i]; QL = V.QL; s1 = V.s1; e1 = V.e1; e3 = V.e3;
			const uint32_t reserved = A.lens[i], fixed = record_bytes(qn, 0u, QL);
			if (reserved < fixed || ((reserved - fixed) & 3u)) fl |= 2u;
			else {
				nc = (reserved - fixed) >> 2;
				uint32_t made;
				if (nc <= (uint32_t)BAM_SMALL_OPS) {
					WordsLds ww{to_lds(&s_words[w][lane * BAM_SLICE]), (uint32_t)BAM_CORE_WORDS + nc};
					made = build_words(A, r, V.F, QL, qn, ww);
					fl |= 1u;
				} else {
					WordsGlobal ww{dst + off, 4u * BAM_CORE_WORDS + qn + 1u, (uint32_t)BAM_CORE_WORDS + nc};
					made = build_words(A, r, V.F, QL, qn, ww);
					fl |= 8u;
				}
				if (made != nc) fl = 2u;
			}
			if (r.dbpos == 0xFFFFFFFFu || r.plus) fl |= 4u;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		const int nrec = (int)(n - base < 64u ? n - base : 64u);
		for (int t = 0; t < nrec; ++t) {
			const uint32_t t_fl = bcast(fl, t), t_qn = bcast(qn, t), t_QL = bcast(QL, t), t_nc = bcast(nc, t);
			const uint32_t t_s1 = bcast(s1, t), t_e1 = bcast(e1, t), t_e3 = bcast(e3, t);
			if (t_fl & 2u) {  // never: the two kernels count the same bytes
				if (lane == 0) atomicOr(&A.hdr->flags, 32u);
				continue;
			}
			const uint8_t *raw = A.raw[A.paired ? ((base + (uint32_t)t) & 1u) : 0u];
			uint8_t *out = dst + bcast(off, t);
			const uint32_t name_at = 4u * BAM_CORE_WORDS, cigar_at = name_at + t_qn + 1u;
			if (t_fl & 1u) {  // the core in front of the name, the CIGAR behind it
				const uint8_t *h = (const uint8_t *)&s_words[w][t * BAM_SLICE];
				const uint32_t hb = 4u * ((uint32_t)BAM_CORE_WORDS + t_nc);
				for (uint32_t k = lane; k < hb; k += 64) out[k < name_at ? k : k + t_qn + 1u] = h[k];
			}
			const uint8_t *label = raw + t_s1 + 1u;
			for (uint32_t k = lane; k <= t_qn; k += 64) out[name_at + k] = k < t_qn ? label[k] : (uint8_t)0;
			const uint8_t *seq = raw + t_e1 + 1u, *qual = raw + t_e3 + 1u;
			const uint32_t nb = (t_QL + 1u) / 2u;
			uint8_t *ps = out + cigar_at + 4u * t_nc, *pq = ps + nb;
			const bool fwd = (t_fl & 4u) != 0;
			const uint8_t *nib = s_nib[fwd ? 0 : 1];
			for (uint32_t j = lane; j < nb; j += 64) {
				const uint32_t k0 = 2u * j, k1 = k0 + 1u;
				const uint32_t hi = nib[seq[fwd ? k0 : t_QL - 1u - k0]];
				const uint32_t lo = k1 < t_QL ? nib[seq[fwd ? k1 : t_QL - 1u - k1]] : 0u;
				ps[j] = (uint8_t)(hi << 4 | lo);
			}
			if (t_QL == 1u && qual[0] == '*') {  // QUAL '*': no qualities
				if (lane == 0) pq[0] = 0xFFu;
			} else
				for (uint32_t k = lane; k < t_QL; k += 64) pq[k] = (uint8_t)(qual[fwd ? k : t_QL - 1u - k] - 33u);
		}
		__builtin_amdgcn_wave_barrier();  // (the next 64 records' words go where these were)
	}
}

}  // namespace

namespace urx {

void bam_len_launch(const SamArgs &A, hipStream_t st) { hipLaunchKernelGGL(bam_len_kernel, dim3(GRID), dim3(256), 0, st, A); }
void bam_launch(const SamArgs &A, hipStream_t st) { hipLaunchKernelGGL(bam_kernel, dim3(GRID), dim3(SAM_WAVES * 64), 0, st, A); }

}  // namespace urx
