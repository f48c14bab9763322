// tags_gpu.hip -- the optional fields NM, MD, AS and RG of a chunk's records on the device (urmapx_text_set_tags; include/urmapx.h
// "Optional fields"), in a translation unit of their own so that the record kernels of text_gpu.hip and bam_gpu.hip are compiled as before.
//
// NM and MD compare every alignment column of a mapped record with the sequence store, along the CIGAR the record prints
// (walk_cigar_runs of text_dev.h: the one place the dangling-M polish lives).  One WAVEFRONT takes one record at a time; within an M run
// lane k holds column 64 s + k of step s: the read byte out of the raw FASTQ chunk (complemented, from the far end, for a minus-strand
// hit: what the record kernel prints), the store byte, both through nibble_of's table (letter_code below); one ballot is the step's 64-bit mismatch mask.  NM adds its
// popcount; every set bit prints "<matches since the last thing printed><reference letter>", whose length each mismatching lane knows
// from the mask alone (the distance to the set bit below it, or to the start of the step plus the count carried in), so a prefix sum over
// the wavefront places all of a step's pieces at once.  The count carries across steps, M runs and I runs; a D run prints the count,
// '^' and its letters, 64 a step.
//
//   tag_len_kernel     the walk without writing: NM, the MD length, the bytes of all fields of the record; slots[i] = lens[i] + those
//                      bytes is what the prefix sum of the record offsets takes, so the record kernel finds room behind every record
//   tag_write_kernel   behind the record kernel: the same walk, the MD text straight into the output (no side buffer, no cap), the
//                      other fields around it; SAM: from the record's '\n' on, a new '\n' behind; BAM: aux bytes behind the record
//                      and block_size raised.  What it wrote must be what tag_len_kernel counted, else the chunk is flagged (32).
//   tags_batch_*       the stage-level entry point (urmapx_tags_batch): reads, results and paths from host arrays through tag_walk
#include <cstring>
#include <vector>

#include "internal.h"
#include "text_dev.h"

namespace {

constexpr int GRID = 2048;
constexpr int TAG_WAVES = 4;

// one record as the walk sees it; the same in every lane of the wavefront
struct TagRec {
	const uint8_t *seq;  // the read as it lies in the FASTQ chunk
	uint32_t QL;
	bool plus;
	const uint8_t *ref;  // the store from the record's first reference base on
	uint32_t ref_room;   // bytes of the store from there to its end
	const urmapx_path_op *ops;
	uint32_t nops;
};

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(v, d, 64);
		if (lane >= d) v += o;
	}
	return v;
}

// The kernels' arguments read where they are used, by vector loads out of the kernel-argument segment.  Taken as scalar values the
// thirty-odd pointers and flags of TagArgs are all loaded in the prologue and stay live across the record loop: with them the two
// text-stage kernels need more scalar registers than a wavefront has (7 / 23 SGPRs go to VGPR lanes), without them 77 / 84 of 102.  An
// address the compiler cannot prove uniform (the zero comes out of a vector move) makes each use a load of its own into a VGPR, of
// which there are plenty.  The struct is the kernel's first and only parameter, so it lies at offset 0 of the segment.
template <class Args>
__device__ __forceinline__ const Args &args_by_vector_loads() {
	uint32_t zero;
	asm("v_mov_b32 %0, 0" : "=v"(zero));
	return *(const Args *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + zero);
}

// nibble_of of text_dev.h -- the 4-bit code of a letter, "=ACMGRSVTWYHKDBN", either case, anything else 15 -- out of a packed table: four
// bits per letter of the alphabet, a to p in one word, q to z in the other.  nibble_of's sixteen compares are sixteen lane masks, and
// with two letters per column the scheduler held thirty-odd of them in scalar registers inside the column loop; this form has three.
__device__ __forceinline__ uint32_t letter_code(uint32_t c) {
	const uint32_t k = (c | 0x20u) - (uint32_t)'a';
	const unsigned long long a_to_p = 0xFFF3FCFFB4FFD2E1ull, q_to_z = 0xFAF97F865Full;
	uint32_t v = (uint32_t)(k < 16u ? a_to_p >> (4u * k) : q_to_z >> ((4u * (k - 16u)) & 63u)) & 15u;
	if (k >= 26u) v = 15u;
	if (c == (uint32_t)'=') v = 0u;
	return v;
}

__device__ __forceinline__ char upper_of(uint32_t c) { return (char)(c - (uint32_t)'a' < 26u ? c - 32u : c); }

// the decimal digits of v at p[0 ..], all by the calling lane; returns how many
__device__ __forceinline__ uint32_t lane_put_uint(char *p, uint32_t v, uint32_t cap) {
	const uint32_t d = dev_digits(v);
	for (uint32_t k = d; k-- > 0;) {
		if (k < cap) p[k] = (char)('0' + v % 10u);
		v /= 10u;
	}
	return d;
}

// the decimal digits of a value every lane holds: lane k writes digit k
__device__ __forceinline__ uint32_t wave_put_uint(char *p, uint32_t v, uint32_t cap) {
	const uint32_t lane = threadIdx.x & 63, d = dev_digits(v);
	if (lane < d && lane < cap) {
		uint32_t x = v;
		for (uint32_t k = d - 1u - lane; k; --k) x /= 10u;
		p[lane] = (char)('0' + x % 10u);
	}
	return d;
}

// a value every lane of the wavefront holds, said to the compiler (it came through vector loads, so the compiler does not know)
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// cigar_ends of text_dev.h without its indexed private arrays (they cost this kernel scratch): what walk_cigar_runs reads of a path --
// how many merged runs, the first three, the last three -- kept in plain variables
__device__ __forceinline__ void tag_cigar_ends(const urmapx_path_op *ops, uint32_t nops, CigarEnds &E) {
	uint32_t N = 0, curlen = 0, f0l = 0, f1l = 0, f2l = 0, l0l = 0, l1l = 0, l2l = 0;
	char cur = 0, f0o = 0, f1o = 0, f2o = 0, l0o = 0, l1o = 0, l2o = 0;
	for (uint32_t i = 0; i <= nops; ++i) {  // (one pass more closes the last run)
		const uint32_t code = i < nops ? ops[i] & 3u : 3u, len = i < nops ? ops[i] >> 2 : 0u;
		const char c = code == 0 ? 'M' : code == 1 ? 'I' : code == 2 ? 'D' : (char)0;
		if (i && cur == c) { curlen += len; continue; }
		if (i) {
			if (N == 0) { f0o = cur; f0l = curlen; }
			else if (N == 1) { f1o = cur; f1l = curlen; }
			else if (N == 2) { f2o = cur; f2l = curlen; }
			l0o = l1o; l0l = l1l; l1o = l2o; l1l = l2l; l2o = cur; l2l = curlen;
			++N;
		}
		cur = c; curlen = len;
	}
	// (the same in every lane, and said so: the rules walk_cigar_runs makes of them are then scalar compares)
	E.N = uni(N); E.chars = 0;
	E.fo[0] = (char)uni(f0o); E.fo[1] = (char)uni(f1o); E.fo[2] = (char)uni(f2o); E.fl[0] = uni(f0l); E.fl[1] = uni(f1l); E.fl[2] = uni(f2l);
	E.lo[0] = (char)uni(l0o); E.lo[1] = (char)uni(l1o); E.lo[2] = (char)uni(l2o); E.ll[0] = uni(l0l); E.ll[1] = uni(l1l); E.ll[2] = uni(l2l);
}

// NM and MD of one record.  WRITE: the MD text goes to md[0, md_cap) (a byte beyond is not stored: the count that comes back gives the
// record away).  nm, md_len: the same value in every lane.
// The emitted runs come from walk_cigar_runs 64 at a time: lane k keeps run base + k, then the wavefront goes through the kept runs, so
// the column work stands in the code once (inside the walk's callback it stood at both places the walk closes a run).  A path of more
// than 64 emitted runs is walked once per 64.
template <bool WRITE>
__device__ __forceinline__ void tag_walk(const TagRec &R_in, const uint8_t *comp, char *md, uint32_t md_cap, uint32_t &nm_out, uint32_t &md_len_out) {
	const uint32_t lane = threadIdx.x & 63;
	uint32_t nm = 0, at = 0, run = 0, q = 0, t = 0;  // at: MD bytes so far; run: matches since the last thing printed; q, t: columns done
	const TagRec &R = R_in;
	CigarEnds E;
	if (R.nops) tag_cigar_ends(R.ops, R.nops, E);
	uint32_t n_runs = 1;  // emitted runs: known once the path has been walked the first time
	for (uint32_t base = 0; base < n_runs; base += 64u) {
		uint32_t my_len = 0, my_op = 0;
		if (R.nops == 0) { my_len = R.QL; my_op = 'M'; }
		else {
			uint32_t idx = 0;
			walk_cigar_runs(R.ops, R.nops, E, [&](uint32_t len, char op) {
				if (idx - base == lane) { my_len = len; my_op = (uint32_t)op; }
				++idx;
			});
			n_runs = uni(idx);
		}
		const uint32_t cnt = n_runs - base < 64u ? n_runs - base : 64u;
		for (uint32_t k = 0; k < cnt; ++k) {
			const uint32_t len = bcast(my_len, (int)k), op = bcast(my_op, (int)k);
			if (op == 'M') {
				for (uint32_t s = 0; s < len; s += 64u) {
					const uint32_t c = s + lane, qi = q + c;
					uint32_t tb = 'N';
					bool mis = false;
					if (c < len && qi < R.QL && t + c < R.ref_room) {
						const uint32_t rb = R.plus ? R.seq[qi] : comp[R.seq[R.QL - 1u - qi]];
						tb = R.ref[t + c];
						const uint32_t a = letter_code(rb), b = letter_code(tb);
						mis = a != b || a == 15u;
					}
					const unsigned long long mask = __ballot(mis);
					const uint32_t cols = len - s < 64u ? len - s : 64u;
					if (mask) {
						nm += (uint32_t)__popcll(mask);
						const unsigned long long below = mask & ((1ull << lane) - 1ull);
						const uint32_t gap = below ? lane - (63u - (uint32_t)__clzll(below)) - 1u : run + lane;
						const uint32_t bytes = mis ? dev_digits(gap) + 1u : 0u;
						const uint32_t inc = wave_incl_scan(bytes);
						if (WRITE && mis) {
							const uint32_t p = at + inc - bytes;
							const uint32_t d = lane_put_uint(md + p, gap, p < md_cap ? md_cap - p : 0u);
							if (p + d < md_cap) md[p + d] = upper_of(tb);
						}
						at += bcast(inc, 63);
						run = cols - 1u - (63u - (uint32_t)__clzll(mask));
					} else
						run += cols;
				}
				q += len; t += len;
			} else if (op == 'I') {
				q += len; nm += len;
			} else {
				at += WRITE ? wave_put_uint(md + at, run, at < md_cap ? md_cap - at : 0u) : dev_digits(run);
				run = 0;
				if (WRITE && lane == 0 && at < md_cap) md[at] = '^';
				at += 1u;
				if (WRITE)
					for (uint32_t c = lane; c < len; c += 64u)
						if (t + c < R.ref_room && at + c < md_cap) md[at + c] = upper_of(R.ref[t + c]);
				at += len; t += len; nm += len;
			}
		}
	}
	at += WRITE ? wave_put_uint(md + at, run, at < md_cap ? md_cap - at : 0u) : dev_digits(run);
	nm_out = nm;
	md_len_out = at;
}

// bytes of an integer aux field's value in the smallest type that holds it (htslib: C S I, or c s i below zero)
__device__ __forceinline__ uint32_t aux_int_bytes(int v) {
	if (v >= 0) return v <= 0xFF ? 1u : v <= 0xFFFF ? 2u : 4u;
	return v >= -128 ? 1u : v >= -32768 ? 2u : 4u;
}
__device__ __forceinline__ char aux_int_type(int v) {
	if (v >= 0) return v <= 0xFF ? 'C' : v <= 0xFFFF ? 'S' : 'I';
	return v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
}
__device__ __forceinline__ uint32_t int_chars(int v) { return v < 0 ? 1u + dev_digits((uint32_t)(-(long long)v)) : dev_digits((uint32_t)v); }

// bytes of a record's fields: text ("\tNM:i:" + digits ...) or aux (tag, type, value)
__device__ __forceinline__ uint32_t field_bytes(const TagArgs &G, bool mapped, uint32_t nm, uint32_t md_len, int score) {
	uint32_t n = 0;
	if (G.bam) {
		if (mapped && (G.mask & URMAPX_TAG_NM)) n += 3u + aux_int_bytes((int)nm);
		if (mapped && (G.mask & URMAPX_TAG_MD)) n += 3u + md_len + 1u;
		if (mapped && (G.mask & URMAPX_TAG_AS)) n += 3u + aux_int_bytes(score);
		if (G.rg_id) n += 3u + G.rg_len + 1u;
	} else {
		if (mapped && (G.mask & URMAPX_TAG_NM)) n += 6u + dev_digits(nm);
		if (mapped && (G.mask & URMAPX_TAG_MD)) n += 6u + md_len;
		if (mapped && (G.mask & URMAPX_TAG_AS)) n += 6u + int_chars(score);
		if (G.rg_id) n += 6u + G.rg_len;
	}
	return n;
}

// the record's lines in its chunk and its window of the store; false: the record names a sequence the index does not have (the record
// length kernels hand such a chunk back)
__device__ __forceinline__ bool tag_rec_of(const TagArgs &G, uint32_t i, const urmapx_result &r, TagRec &R) {
	const SamArgs &A = G.A;
	const uint32_t side = A.paired ? (i & 1u) : 0u, rec = A.paired ? (i >> 1) : i;
	const uint32_t *ends = A.ends[side];
	const uint32_t e1 = ends[4 * rec], e2 = ends[4 * rec + 1];
	R.seq = A.raw[side] + e1 + 1u;
	R.QL = e2 - (e1 + 1u);
	R.plus = r.plus != 0;
	R.ops = A.ops + r.path_off;
	R.nops = r.path_nops;
	if (r.seq_index >= A.seq_count) return false;
	const unsigned long long at = (unsigned long long)G.seq_offs[r.seq_index] + r.coord;
	R.ref = G.store + at;
	R.ref_room = at < G.store_size ? (uint32_t)(G.store_size - at) : 0u;
	return true;
}

__global__ __launch_bounds__(TAG_WAVES * 64) void tag_len_kernel(TagArgs) {
	const TagArgs &G = args_by_vector_loads<TagArgs>();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t n = G.A.hdr->n_reads;
	const uint32_t wave = blockIdx.x * TAG_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * TAG_WAVES;
	for (uint32_t i = wave; i < n; i += n_waves) {
		const urmapx_result r = G.A.results[i];
		const bool mapped = r.dbpos != 0xFFFFFFFFu;
		uint32_t nm = 0, md_len = 0;
		TagRec R;
		if (mapped && (G.mask & (URMAPX_TAG_NM | URMAPX_TAG_MD)) && tag_rec_of(G, i, r, R)) tag_walk<false>(R, G.A.comp, nullptr, 0u, nm, md_len);
		if (lane == 0) {
			const uint32_t tl = field_bytes(G, mapped, nm, md_len, r.score);
			G.nm[i] = nm; G.md_len[i] = md_len; G.tag_len[i] = tl;
			G.slots[i] = G.A.lens[i] + tl;
		}
	}
}

// n <= 8 bytes of `bytes` (the first in its low byte) at p, one per lane
__device__ __forceinline__ void wave_put_bytes(char *p, unsigned long long bytes, uint32_t n) {
	const uint32_t lane = threadIdx.x & 63;
	if (lane < n) p[lane] = (char)(bytes >> (8u * lane));
}
__device__ __forceinline__ unsigned long long text_prefix(char a, char b, char type) {  // "\tXX:t:"
	return (unsigned long long)'\t' | (unsigned long long)(uint8_t)a << 8 | (unsigned long long)(uint8_t)b << 16 | (unsigned long long)':' << 24 |
	       (unsigned long long)(uint8_t)type << 32 | (unsigned long long)':' << 40;
}
__device__ __forceinline__ uint32_t wave_put_int(char *p, int v) {
	if (v >= 0) return wave_put_uint(p, (uint32_t)v, 16u);
	if ((threadIdx.x & 63) == 0) p[0] = '-';
	return 1u + wave_put_uint(p + 1, (uint32_t)(-(long long)v), 16u);
}
__device__ __forceinline__ uint32_t wave_put_aux_int(char *p, char a, char b, int v) {  // tag, type, little-endian value
	const uint32_t nb = aux_int_bytes(v);
	wave_put_bytes(p, (unsigned long long)(uint8_t)a | (unsigned long long)(uint8_t)b << 8 | (unsigned long long)(uint8_t)aux_int_type(v) << 16 |
	                      (unsigned long long)(uint32_t)v << 24, 3u + nb);
	return 3u + nb;
}

__global__ __launch_bounds__(TAG_WAVES * 64) void tag_write_kernel(TagArgs) {
	const TagArgs &G = args_by_vector_loads<TagArgs>();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t n = G.A.hdr->n_reads;
	const uint32_t wave = blockIdx.x * TAG_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * TAG_WAVES;
	for (uint32_t i = wave; i < n; i += n_waves) {
		const uint32_t tl = G.tag_len[i];
		if (tl == 0) continue;
		const urmapx_result r = G.A.results[i];
		const bool mapped = r.dbpos != 0xFFFFFFFFu;
		const uint32_t base_len = G.A.lens[i], nm = G.nm[i], md_len = G.md_len[i];
		char *const rec = G.A.sam + G.A.rec_offs[i];
		char *p = rec + (G.bam ? base_len : base_len - 1u);  // SAM: the fields begin where the record kernel put the '\n'
		uint32_t made = 0, md_made = md_len, nm_made = nm;
		const bool walk = mapped && (G.mask & URMAPX_TAG_MD);
		if (mapped && (G.mask & URMAPX_TAG_NM)) {
			if (G.bam) made += wave_put_aux_int(p + made, 'N', 'M', (int)nm);
			else { wave_put_bytes(p + made, text_prefix('N', 'M', 'i'), 6u); made += 6u; made += wave_put_uint(p + made, nm, 16u); }
		}
		if (walk) {
			if (G.bam) { wave_put_bytes(p + made, (unsigned long long)'M' | (unsigned long long)'D' << 8 | (unsigned long long)'Z' << 16, 3u); made += 3u; }
			else { wave_put_bytes(p + made, text_prefix('M', 'D', 'Z'), 6u); made += 6u; }
			TagRec R;
			if (tag_rec_of(G, i, r, R)) tag_walk<true>(R, G.A.comp, p + made, md_len, nm_made, md_made);
			else md_made = 0xFFFFFFFFu;
			made += md_len;
			if (G.bam) { if (lane == 0) p[made] = 0; made += 1u; }
		}
		if (mapped && (G.mask & URMAPX_TAG_AS)) {
			if (G.bam) made += wave_put_aux_int(p + made, 'A', 'S', r.score);
			else { wave_put_bytes(p + made, text_prefix('A', 'S', 'i'), 6u); made += 6u; made += wave_put_int(p + made, r.score); }
		}
		if (G.rg_id) {
			if (G.bam) { wave_put_bytes(p + made, (unsigned long long)'R' | (unsigned long long)'G' << 8 | (unsigned long long)'Z' << 16, 3u); made += 3u; }
			else { wave_put_bytes(p + made, text_prefix('R', 'G', 'Z'), 6u); made += 6u; }
			for (uint32_t k = lane; k < G.rg_len; k += 64u) p[made + k] = G.rg_id[k];
			made += G.rg_len;
			if (G.bam) { if (lane == 0) p[made] = 0; made += 1u; }
		}
		if (G.bam) wave_put_bytes(rec, (unsigned long long)(base_len + tl - 4u), 4u);  // block_size covers the aux fields
		else if (lane == 0) p[tl] = '\n';
		// never: the two passes walk the same columns
		if ((made != tl || md_made != md_len || nm_made != nm) && lane == 0) atomicOr(&G.A.hdr->flags, 32u);
	}
}

// ---- the stage-level entry point: reads, results and paths as urmapx_map_se has them ----
struct BatchArgs {
	const uint8_t *bases;
	const uint64_t *offs;
	uint32_t n;
	const urmapx_result *results;
	const urmapx_path_op *ops;
	const uint8_t *comp, *store;
	const uint32_t *seq_offs;
	uint32_t store_size, seq_count;
	uint32_t *nm, *md_len;
	const uint64_t *md_offs;  // write pass
	char *md;
};

__device__ __forceinline__ bool batch_rec_of(const BatchArgs &B, uint32_t i, const urmapx_result &r, TagRec &R) {
	R.seq = B.bases + B.offs[i];
	R.QL = (uint32_t)(B.offs[i + 1] - B.offs[i]);
	R.plus = r.plus != 0;
	R.ops = B.ops + r.path_off;
	R.nops = r.path_nops;
	if (r.seq_index >= B.seq_count) return false;
	const unsigned long long at = (unsigned long long)B.seq_offs[r.seq_index] + r.coord;
	R.ref = B.store + at;
	R.ref_room = at < B.store_size ? (uint32_t)(B.store_size - at) : 0u;
	return true;
}

template <bool WRITE>
__global__ __launch_bounds__(TAG_WAVES * 64) void tags_batch_kernel(BatchArgs) {
	const BatchArgs &B = args_by_vector_loads<BatchArgs>();
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = blockIdx.x * TAG_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * TAG_WAVES;
	for (uint32_t i = wave; i < B.n; i += n_waves) {
		const urmapx_result r = B.results[i];
		uint32_t nm = 0, md_len = 0;
		TagRec R;
		if (r.dbpos != 0xFFFFFFFFu && batch_rec_of(B, i, r, R)) {
			if (WRITE) tag_walk<true>(R, B.comp, B.md + B.md_offs[i], (uint32_t)(B.md_offs[i + 1] - B.md_offs[i]), nm, md_len);
			else tag_walk<false>(R, B.comp, nullptr, 0u, nm, md_len);
		}
		if (!WRITE && lane == 0) { B.nm[i] = nm; B.md_len[i] = md_len; }
	}
}

// the bytes of the store under a list of spans, back to back: one wavefront per span at a time
__global__ __launch_bounds__(256) void span_gather_kernel(const uint8_t *store, const uint64_t *starts, const uint64_t *out_offs, uint32_t n, uint8_t *out) {
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
	for (uint32_t i = wave; i < n; i += n_waves) {
		const uint8_t *src = store + starts[i];
		uint8_t *dst = out + out_offs[i];
		const uint64_t len = out_offs[i + 1] - out_offs[i];
		for (uint64_t k = lane; k < len; k += 64u) dst[k] = src[k];
	}
}

}  // namespace

namespace urx {

void tag_len_launch(const TagArgs &G, hipStream_t st) { hipLaunchKernelGGL(tag_len_kernel, dim3(GRID), dim3(TAG_WAVES * 64), 0, st, G); }
void tag_write_launch(const TagArgs &G, hipStream_t st) { hipLaunchKernelGGL(tag_write_kernel, dim3(GRID), dim3(TAG_WAVES * 64), 0, st, G); }

}  // namespace urx

namespace urx { const unsigned char *complement_table(); }

extern "C" {

int urmapx_tags_batch(urmapx_ctx *C, const uint8_t *bases, const uint64_t *offs, uint32_t n, const urmapx_result *results,
                      const urmapx_path_op *path_ops, size_t path_n, unsigned mask, uint32_t *nm, uint8_t *tagged, char *md, size_t md_cap,
                      uint64_t *md_offs, size_t *md_used) {
	if (!C || !md_offs || !md_used || (mask & ~URMAPX_TAG_ALL) || (n && (!bases || !offs || !results || !nm || !tagged))) return URMAPX_E_ARG;
	*md_used = 0;
	md_offs[0] = 0;
	if (n == 0) return URMAPX_OK;
	const IndexStore S = index_store(ctx_index(C));
	if (!S.d_seq || !S.d_seq_offsets || S.device != ctx_device(C)) return URMAPX_E_ARG;
	const urmapx_index *I = ctx_index(C);
	// every alignment inside its read and its sequence: the kernels walk what the results say
	for (uint32_t i = 0; i < n; ++i) {
		const urmapx_result &r = results[i];
		tagged[i] = r.dbpos != 0xFFFFFFFFu ? 1 : 0;
		if (r.dbpos == 0xFFFFFFFFu) continue;
		const uint64_t QL = offs[i + 1] - offs[i];
		if (offs[i + 1] < offs[i] || QL > 0xFFFFFFFFull || r.seq_index >= S.seq_count) return URMAPX_E_ARG;
		uint64_t qspan = 0, tspan = 0;
		if (r.path_nops == 0) qspan = tspan = QL;
		else {
			if (!path_ops || (uint64_t)r.path_off + r.path_nops > path_n) return URMAPX_E_ARG;
			for (uint32_t k = 0; k < r.path_nops; ++k) {
				const uint32_t code = path_ops[r.path_off + k] & 3u, len = path_ops[r.path_off + k] >> 2;
				if (code == 3u) return URMAPX_E_ARG;
				if (code != 2u) qspan += len;  // path I: target base against a gap
				if (code != 1u) tspan += len;  // path D: query base against a gap
			}
		}
		if (qspan != QL || (uint64_t)r.coord + tspan > urmapx_index_seq_length(I, r.seq_index)) return URMAPX_E_ARG;
	}
	HIP_TRY(hipSetDevice(ctx_device(C)));
	hipStream_t st = ctx_stream(C);
	const uint64_t total = offs[n];
	DevBuf<uint8_t> d_bases, d_comp;
	DevBuf<uint64_t> d_offs, d_mdoffs;
	DevBuf<urmapx_result> d_res;
	DevBuf<urmapx_path_op> d_ops;
	DevBuf<uint32_t> d_nm, d_mdlen;
	DevBuf<char> d_md;
	auto release = [&]() {
		d_bases.release(); d_comp.release(); d_offs.release(); d_mdoffs.release(); d_res.release(); d_ops.release(); d_nm.release(); d_mdlen.release(); d_md.release();
	};
	int rc = d_bases.ensure((size_t)total + 64);
	if (!rc) rc = d_comp.ensure(256);
	if (!rc) rc = d_offs.ensure((size_t)n + 1);
	if (!rc) rc = d_mdoffs.ensure((size_t)n + 1);
	if (!rc) rc = d_res.ensure(n);
	if (!rc) rc = d_ops.ensure(path_n + 1);
	if (!rc) rc = d_nm.ensure(n);
	if (!rc) rc = d_mdlen.ensure(n);
	if (rc) { release(); return rc; }
	std::vector<uint32_t> h_mdlen(n);
	auto run = [&]() -> int {
		if (total) HIP_TRY(hipMemcpyAsync(d_bases.p, bases, (size_t)total, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_comp.p, complement_table(), 256, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_offs.p, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d_res.p, results, (size_t)n * sizeof(urmapx_result), hipMemcpyHostToDevice, st));
		if (path_n) HIP_TRY(hipMemcpyAsync(d_ops.p, path_ops, path_n * sizeof(urmapx_path_op), hipMemcpyHostToDevice, st));
		BatchArgs B;
		B.bases = d_bases.p; B.offs = d_offs.p; B.n = n; B.results = d_res.p; B.ops = d_ops.p; B.comp = d_comp.p; B.store = S.d_seq;
		B.seq_offs = S.d_seq_offsets; B.store_size = S.seq_data_size; B.seq_count = S.seq_count; B.nm = d_nm.p; B.md_len = d_mdlen.p;
		B.md_offs = nullptr; B.md = nullptr;
		const uint32_t blocks = n < (uint32_t)GRID * TAG_WAVES ? (n + TAG_WAVES - 1) / TAG_WAVES : (uint32_t)GRID;
		hipLaunchKernelGGL(tags_batch_kernel<false>, dim3(blocks), dim3(TAG_WAVES * 64), 0, st, B);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(nm, d_nm.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(h_mdlen.data(), d_mdlen.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (uint32_t i = 0; i < n; ++i) md_offs[i + 1] = md_offs[i] + ((mask & URMAPX_TAG_MD) && tagged[i] ? h_mdlen[i] : 0u);
		*md_used = (size_t)md_offs[n];
		if (!(mask & URMAPX_TAG_NM))
			for (uint32_t i = 0; i < n; ++i) nm[i] = 0;
		if (md_offs[n] == 0) return URMAPX_OK;
		if (!md || md_cap < md_offs[n]) return URMAPX_E_ARG;
		int rc2 = d_md.ensure((size_t)md_offs[n] + 64);
		if (rc2) return rc2;
		HIP_TRY(hipMemcpyAsync(d_mdoffs.p, md_offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
		B.md_offs = d_mdoffs.p; B.md = d_md.p;
		hipLaunchKernelGGL(tags_batch_kernel<true>, dim3(blocks), dim3(TAG_WAVES * 64), 0, st, B);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(md, d_md.p, (size_t)md_offs[n], hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return URMAPX_OK;
	};
	rc = run();
	release();
	return rc;
}

int urmapx_index_fetch_spans(const urmapx_index *I, const uint64_t *starts, const uint32_t *lens, uint32_t n, uint8_t *out) {
	if (!I || (n && (!starts || !lens || !out))) return URMAPX_E_ARG;
	const IndexStore S = index_store(I);
	std::vector<uint64_t> out_offs((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) {
		if (starts[i] > S.seq_data_size || lens[i] > S.seq_data_size - starts[i]) return URMAPX_E_ARG;
		out_offs[i + 1] = out_offs[i] + lens[i];
	}
	if (n == 0 || out_offs[n] == 0) return URMAPX_OK;
	if (S.h_seq) {
		for (uint32_t i = 0; i < n; ++i) memcpy(out + out_offs[i], S.h_seq + starts[i], lens[i]);
		return URMAPX_OK;
	}
	if (!S.d_seq || S.device < 0) return URMAPX_E_ARG;
	HIP_TRY(hipSetDevice(S.device));
	DevBuf<uint64_t> d_starts, d_offs;
	DevBuf<uint8_t> d_out;
	int rc = d_starts.ensure(n);
	if (!rc) rc = d_offs.ensure((size_t)n + 1);
	if (!rc) rc = d_out.ensure((size_t)out_offs[n]);
	auto run = [&]() -> int {
		HIP_TRY(hipMemcpy(d_starts.p, starts, (size_t)n * 8, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_offs.p, out_offs.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
		const uint32_t blocks = n < 4096u * 4u ? (n + 3u) / 4u : 4096u;
		hipLaunchKernelGGL(span_gather_kernel, dim3(blocks), dim3(256), 0, nullptr, S.d_seq, d_starts.p, d_offs.p, n, d_out.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(out, d_out.p, (size_t)out_offs[n], hipMemcpyDeviceToHost));
		return URMAPX_OK;
	};
	if (!rc) rc = run();
	d_starts.release(); d_offs.release(); d_out.release();
	return rc;
}

}  // extern "C"
