// pileup.hip -- SNV candidate sites of BAM records on the device (urmapx_bam_pileup, and the pileup step of urmapx_bam_sort_with; the
// rule is in include/urmapx.h "Pileup", the site entry, the sizes and the memory sum in pileup.h, the host version and the formatter
// in pileup_host.cpp).
//
// The counters are one uint4 (A, C, G, T) per reference column; reference r owns entries base[r] .. base[r] + l_ref - 1.  All indices
// are 64 bits wide.  No counter wraps: fewer than 2^31 records, one add per record and column at the most.
//
//   pileup_count_kernel  a persistent grid of workgroups of four wavefronts; a WAVEFRONT takes one record at a time.  Six lanes load
//                        the core words, which become scalars (readlane), so the whole filter is uniform.  The CIGAR is taken 64 ops
//                        a step, lane = op: shuffle scans of the reference-consuming and of the query-consuming lengths give every op
//                        both cursors, and a third scan, of the covered lengths clipped to l_ref and l_seq, lays the covered bases of
//                        the step end to end.  They are walked 64 a step, lane = base: a binary search over the third scan (six
//                        shuffles) finds the lane's op, then one SEQ nibble, one QUAL byte, one no-return atomicAdd on the lane's own
//                        column entry.  The 64 lanes of an M run fall on 64 consecutive 16-byte entries, a dword each.  A step costs
//                        the same whether its bases come from one op or from 64, so a record of n ops and b covered bases takes
//                        ceil(n / 64) op steps and at most ceil(n / 64) + b / 64 base steps: no lane ever walks a CIGAR alone.
//   site_count / block_scan / site_write   a segment of columns at a time, a column a thread: the 16 bytes of counters and the
//                        reference letter (one binary search per wavefront for the reference where all its columns share it),
//                        rule 3, the workgroup's count; the counts are scanned; the second kernel finds the same flags again and
//                        writes the sites whose rank falls into the slice asked for as entries of 24 bytes, in column order.
#include "pileup_dev.h"
#include "block_scan_dev.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

#include "depth.h"

using namespace urx::bamsort;
using namespace urx::pileup;
using urx::devscan::block_scan_kernel;
using urx::devscan::BS_NT;

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr uint32_t PNT = urx::pileup::NT;
// CIGAR ops as bits 1 << op: M = X cover; M D N = X advance the reference cursor; M I S = X the query cursor
constexpr uint32_t OPS_COVER = 1u << 0 | 1u << 7 | 1u << 8, OPS_REF = OPS_COVER | 1u << 2 | 1u << 3, OPS_QUERY = OPS_COVER | 1u << 1 | 1u << 4;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_word(uint32_t v, uint32_t from) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)from); }
__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t from) { return (uint32_t)__shfl((int)v, (int)from, 64); }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t from) { return (uint64_t)shfl32((uint32_t)(v >> 32), from) << 32 | shfl32((uint32_t)v, from); }
// the inclusive sums of v over the lanes of a wavefront
__device__ __forceinline__ uint32_t wave_scan32(uint32_t v, uint32_t lane) {
	for (uint32_t by = 1; by < 64u; by <<= 1) {
		const uint32_t t = (uint32_t)__shfl_up((int)v, by, 64);
		if (lane >= by) v += t;
	}
	return v;
}
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, uint32_t lane) {
	for (uint32_t by = 1; by < 64u; by <<= 1) {
		const uint64_t t = (uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), by, 64) << 32 | (uint32_t)__shfl_up((int)(uint32_t)v, by, 64);
		if (lane >= by) v += t;
	}
	return v;
}

// ---- counting ----
__global__ __launch_bounds__(PNT) void pileup_count_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action,
                                                           uint32_t min_mapq, uint32_t min_baseq, uint32_t n_ref, const uint64_t *ref_base, uint32_t *cnt,
                                                           unsigned long long *stat) {
	const uint32_t lane = threadIdx.x & 63u, wave = uni(threadIdx.x >> 6), n = i1 - i0;
	uint32_t counted = 0;  // records of this wavefront that passed rule 1
	for (uint64_t k = (uint64_t)blockIdx.x * WAVES + wave; k < n; k += (uint64_t)gridDim.x * WAVES) {
		const uint64_t i = i0 + k, at = off[i], len = off[i + 1] - at;
		const uint8_t *r = rec + (at - base);
		const uint32_t hw = lane < 6u ? load_u32(r + 4u * lane) : 0u;
		const uint32_t ref = lane_word(hw, 1), p = lane_word(hw, 2), w3 = lane_word(hw, 3), w4 = lane_word(hw, 4), l_seq = lane_word(hw, 5);
		uint32_t flag = w4 >> 16;
		if (action) {
			const uint8_t a = action[i];
			if (a == MD_SET) flag |= 0x400u;
			else if (a == MD_CLEAR) flag &= ~0x400u;
		}
		flag = uni(flag);
		const uint32_t mapq = w3 >> 8 & 0xFFu, l_name = w3 & 0xFFu, n_cigar = w4 & 0xFFFFu;
		if (!(ref < n_ref) || (p >> 31) || (flag & 0x704u) || mapq < min_mapq) continue;
		++counted;
		if ((uint64_t)CORE + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + l_seq > len) continue;
		const uint8_t *cig = r + CORE + l_name, *seq = cig + 4ull * n_cigar, *qual = seq + ((uint64_t)l_seq + 1u) / 2u;
		if (l_seq == 0) continue;
		const bool no_qual = uni(qual[0]) == 0xFFu;
		const uint64_t b = ref_base[ref], l_ref = ref_base[ref + 1] - b;
		uint64_t x_at = p, q_at = 0;  // both cursors in front of op o0
		for (uint32_t o0 = 0; o0 < n_cigar; o0 += 64u) {
			const uint32_t o = o0 + lane;
			const bool valid = o < n_cigar;
			const uint32_t w = valid ? load_u32(cig + 4ull * o) : 0u, L = w >> 4;
			const uint32_t kind = valid ? 1u << (w & 15u) : 0u;  // the op as one bit: what it does is a mask away
			const bool cov = (kind & OPS_COVER) != 0u;
			const uint64_t adv_x = kind & OPS_REF ? (uint64_t)L : 0u, adv_q = kind & OPS_QUERY ? (uint64_t)L : 0u;
			const uint64_t inc_x = wave_scan64(adv_x, lane), inc_q = wave_scan64(adv_q, lane);
			const uint64_t my_x = x_at + inc_x - adv_x, my_q = q_at + inc_q - adv_q;
			// the covered bases of the op that lie on the reference and in the read (their sum over a record is at most l_seq)
			uint64_t room = L;
			if (!cov || my_x >= l_ref || my_q >= l_seq) room = 0;
			else {
				if (l_ref - my_x < room) room = l_ref - my_x;
				if ((uint64_t)l_seq - my_q < room) room = (uint64_t)l_seq - my_q;
			}
			const uint32_t eff = (uint32_t)room, inc_e = wave_scan32(eff, lane);
			const uint32_t total = lane_word(inc_e, 63);
			for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
				const bool in = t0 + lane < total;
				const uint32_t t = in ? t0 + lane : total - 1u;
				uint32_t s = 0;  // the op of base t: the ops in front of it whose bases end at or below t
				for (uint32_t step = 32; step; step >>= 1) {
					const uint32_t v = shfl32(inc_e, s + step - 1u);
					if (v <= t) s += step;
				}
				const uint32_t j = t - (shfl32(inc_e, s) - shfl32(eff, s));  // its place in the op
				const uint64_t bq = shfl64(my_q, s) + j, col = shfl64(my_x, s) + j;
				if (in) {
					const uint32_t code = bq & 1u ? seq[bq >> 1] & 15u : seq[bq >> 1] >> 4, bb = base_of_code(code);
					if (bb < 4u && (no_qual || qual[bq] >= min_baseq)) atomicAdd(cnt + (4ull * (b + col) + bb), 1u);
				}
			}
			x_at += shfl64(inc_x, 63);
			q_at += shfl64(inc_q, 63);
		}
	}
	if (lane == 0 && counted) atomicAdd(stat, (unsigned long long)counted);
}

// ---- the sites ----
// the reference that owns column g: the largest r below n_ref with base[r] <= g (g < base[n_ref], n_ref >= 1)
__device__ __forceinline__ uint32_t ref_of(const uint64_t *base, uint32_t n_ref, uint64_t g) {
	uint32_t lo = 0, hi = n_ref;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (base[mid] <= g) lo = mid; else hi = mid;
	}
	return lo;
}
// Column g of the segment that ends at s1: is it a site, and if so its entry.  Every lane of a wavefront calls this
__device__ __forceinline__ bool site_at(const uint4 *cnt, const uint8_t *seq, const uint64_t *seq_at, const uint64_t *base, uint32_t n_ref, uint64_t g, uint64_t s1,
                                        uint32_t min_alt, uint32_t min_pct, Site &S) {
	// the references of the wavefront's first and last column, the same for all lanes; a lane searches itself only between two references
	const uint64_t g_first = g - (threadIdx.x & 63u), g_last = g_first + 63u < s1 ? g_first + 63u : s1 - 1u;
	if (g_first >= s1) return false;
	const uint32_t r_first = ref_of(base, n_ref, g_first), r_last = ref_of(base, n_ref, g_last);
	if (g >= s1) return false;
	const uint4 c = cnt[g];
	const uint32_t v[4] = {c.x, c.y, c.z, c.w};
	if (!(c.x | c.y | c.z | c.w)) return false;
	const uint32_t r = r_first == r_last ? r_first : ref_of(base, n_ref, g);
	const uint32_t ref = base_of_letter(seq[seq_at[r] + (g - base[r])]);
	if (ref > 3u || !alt_mask(v, ref, min_alt, min_pct)) return false;
	S.column = g | (uint64_t)ref << REF_SHIFT;
	S.cnt[0] = c.x; S.cnt[1] = c.y; S.cnt[2] = c.z; S.cnt[3] = c.w;
	return true;
}

// the segment [s0, s1): workgroup b looks at the PNT columns from s0 + b * PNT on
__global__ __launch_bounds__(PNT) void site_count_kernel(const uint4 *cnt, const uint8_t *seq, const uint64_t *seq_at, const uint64_t *base, uint32_t n_ref, uint64_t s0,
                                                         uint64_t s1, uint32_t min_alt, uint32_t min_pct, uint32_t *bcount) {
	__shared__ uint32_t s_w[WAVES];
	Site S;
	const bool site = site_at(cnt, seq, seq_at, base, n_ref, s0 + (uint64_t)blockIdx.x * PNT + threadIdx.x, s1, min_alt, min_pct, S);
	const uint32_t found = (uint32_t)__popcll(__ballot(site));
	if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = found;
	__syncthreads();
	if (threadIdx.x == 0) bcount[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// boff: the scanned counts (one entry more: the next workgroup's, or the total).  The sites of ranks [w0, w1) within the segment go to
// out[rank - w0]
__global__ __launch_bounds__(PNT) void site_write_kernel(const uint4 *cnt, const uint8_t *seq, const uint64_t *seq_at, const uint64_t *base, uint32_t n_ref, uint64_t s0,
                                                         uint64_t s1, uint32_t min_alt, uint32_t min_pct, const uint32_t *boff, uint32_t w0, uint32_t w1, Site *out) {
	__shared__ uint32_t s_w[WAVES];
	const uint32_t b0 = boff[blockIdx.x], b1 = boff[blockIdx.x + 1];
	if (b1 <= w0 || b0 >= w1 || b0 == b1) return;  // (the same for the whole workgroup)
	Site S;
	const bool site = site_at(cnt, seq, seq_at, base, n_ref, s0 + (uint64_t)blockIdx.x * PNT + threadIdx.x, s1, min_alt, min_pct, S);
	const unsigned long long m = __ballot(site);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t rank = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
	for (uint32_t w = 0; w < wave; ++w) rank += s_w[w];
	if (site && rank >= w0 && rank < w1) out[rank - w0] = S;
}

}  // namespace

namespace urx {
namespace pileup {

int PileupOwn::begin(uint32_t n_ref_, const uint32_t *lens, uint64_t columns_, const uint8_t *const *seqs, const uint8_t *d_store, const uint64_t *store_at) {
	n_ref = n_ref_;
	columns = columns_;
	segment = segment_columns();
	slice = slice_sites();
	int dev = 0, cus = 0;
	HIP_TRY(hipGetDevice(&dev));
	HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
	blocks = cus > 0 ? 8u * (uint32_t)cus : 8u;  // eight workgroups of four wavefronts a compute unit
	if (const uint32_t most = test_blocks()) blocks = std::min(blocks, most);
	const uint64_t seg_blocks = ((columns < segment ? columns : segment) + PNT - 1) / PNT;
	int rc;
	if ((rc = cnt.alloc((size_t)columns)) || (rc = base.alloc((size_t)n_ref + 1)) || (rc = seq_at.alloc((size_t)n_ref + 1)) || (rc = bcount.alloc((size_t)seg_blocks + 1)) ||
	    (rc = sites[0].alloc(slice)) || (rc = sites[1].alloc(slice)) || (rc = stat.alloc(1)))
		return rc;
	if (seqs && (rc = bases.alloc((size_t)columns))) return rc;
	std::vector<uint64_t> h_base((size_t)n_ref + 1, 0), h_at((size_t)n_ref + 1, 0);
	for (uint32_t r = 0; r < n_ref; ++r) {
		h_base[r + 1] = h_base[r] + lens[r];
		h_at[r] = seqs ? h_base[r] : store_at[r];
	}
	if (h_base[n_ref] != columns) return URMAPX_E_ARG;
	HIP_TRY(hipMemcpy(base.p, h_base.data(), h_base.size() * 8, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(seq_at.p, h_at.data(), h_at.size() * 8, hipMemcpyHostToDevice));
	if (seqs) {
		for (uint32_t r = 0; r < n_ref; ++r)
			if (lens[r]) HIP_TRY(hipMemcpy(bases.p + h_base[r], seqs[r], lens[r], hipMemcpyHostToDevice));
		seq = bases.p;
	} else
		seq = d_store;
	HIP_TRY(hipMemset(cnt.p, 0, (size_t)(columns ? columns : 1) * sizeof(uint4)));
	HIP_TRY(hipMemset(stat.p, 0, 8));
	return URMAPX_OK;
}

int pileup_count(const PileupOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, const Rule &R,
                 hipStream_t stream) {
	if (i1 <= i0 || W.n_ref == 0) return URMAPX_OK;
	const uint32_t want = (i1 - i0 + WAVES - 1) / WAVES;  // a wavefront a record
	hipLaunchKernelGGL(pileup_count_kernel, dim3(std::min(W.blocks, want)), dim3(PNT), 0, stream, rec, base, off, i0, i1, action, R.min_mapq, R.min_baseq, W.n_ref,
	                   (const uint64_t *)W.base.p, (uint32_t *)W.cnt.p, W.stat.p);
	return URMAPX_OK;
}

int pileup_finish(PileupOwn &W, const char *const *names, const uint32_t *lens, const Rule &R, const char *command, urmapx_pileup_result *out) {
	HIP_TRY(hipDeviceSynchronize());
	unsigned long long counted = 0;
	HIP_TRY(hipMemcpy(&counted, W.stat.p, 8, hipMemcpyDeviceToHost));
	out->records = counted;

	// Segment after segment: its sites are counted, then written a slice at a time: slice k on stream k & 1 into sites[k & 1] and copied
	// to a page-locked buffer of its own while slice k + 1 is written on the other stream; a buffer's entries are appended to the list
	// when its stream is next waited for
	const uint32_t slice = W.slice;
	Pinned h_sites[2];
	TwoStreams st;
	std::vector<Site> list;
	int rc;
	if ((rc = h_sites[0].alloc((size_t)slice * sizeof(Site))) || (rc = h_sites[1].alloc((size_t)slice * sizeof(Site))) || (rc = st.create())) return rc;
	uint64_t pending[2] = {0, 0}, n_slices = 0;
	auto collect = [&](int b) -> int {  // what stream b was copying
		const auto t0 = Clock::now();
		HIP_TRY(hipStreamSynchronize(st.s[b]));
		const Site *from = (const Site *)h_sites[b].p;
		list.insert(list.end(), from, from + pending[b]);
		pending[b] = 0;
		out->copy_s += since(t0);
		return URMAPX_OK;
	};
	const uint4 *cnt = W.cnt.p;
	const uint64_t *base = W.base.p, *seq_at = W.seq_at.p;
	for (uint64_t s0 = 0; s0 < W.columns; s0 += W.segment) {
		const uint64_t s1 = std::min(s0 + W.segment, W.columns);
		auto t = Clock::now();
		const uint32_t blocks = (uint32_t)((s1 - s0 + PNT - 1) / PNT);
		uint32_t found = 0;
		hipLaunchKernelGGL(site_count_kernel, dim3(blocks), dim3(PNT), 0, nullptr, cnt, W.seq, seq_at, base, W.n_ref, s0, s1, R.min_alt, R.min_pct, W.bcount.p);
		hipLaunchKernelGGL((block_scan_kernel<uint32_t>), dim3(1), dim3(BS_NT), 0, nullptr, (const uint32_t *)W.bcount.p, W.bcount.p, blocks, 1);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpy(&found, W.bcount.p + blocks, 4, hipMemcpyDeviceToHost));
		if (found > s1 - s0) return URMAPX_E_NODEVICE;
		out->sites_s += since(t);
		for (uint32_t w0 = 0; w0 < found; w0 += slice) {
			const uint32_t w1 = (uint32_t)std::min<uint64_t>((uint64_t)w0 + slice, found);
			const int b = (int)(n_slices & 1u);
			if ((rc = collect(b))) return rc;
			t = Clock::now();
			hipLaunchKernelGGL(site_write_kernel, dim3(blocks), dim3(PNT), 0, st.s[b], cnt, W.seq, seq_at, base, W.n_ref, s0, s1, R.min_alt, R.min_pct,
			                   (const uint32_t *)W.bcount.p, w0, w1, W.sites[b].p);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(h_sites[b].p, W.sites[b].p, (size_t)(w1 - w0) * sizeof(Site), hipMemcpyDeviceToHost, st.s[b]));
			pending[b] = w1 - w0;
			++n_slices;
			out->sites_s += since(t);
		}
		// the counts are written again by the next segment: their readers end first (the older slice first)
		for (uint64_t k = n_slices >= 2 ? n_slices - 2 : 0; k < n_slices; ++k)
			if ((rc = collect((int)(k & 1u)))) return rc;
	}
	const auto t = Clock::now();
	rc = format_sites(list.data(), list.size(), W.n_ref, names, lens, R, command, out);
	out->format_s = since(t);
	return rc;
}

uint64_t PileupBeside::resident_bytes() const { return urx::pileup::resident_bytes(columns, n_ref, segment_columns(), slice_sites(), !seqs); }
int PileupBeside::begin(uint32_t) { return W.begin(n_ref, lens, columns, seqs, d_store, store_at); }
int PileupBeside::count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) {
	return pileup_count(W, at, base, off, i0, i1, action, R, stream);
}
int PileupBeside::finish() { return pileup_finish(W, names, lens, R, command, out); }
void PileupBeside::free_result() { urmapx_pileup_free(out); }

}  // namespace pileup
}  // namespace urx

extern "C" {

int urmapx_bam_pileup(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint8_t *const *seqs,
                      const uint64_t *starts, size_t n_starts, const urmapx_pileup_opts *opts, const char *command, urmapx_pileup_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t columns = 0;
	Rule R;
	int rc = check_input(n_ref, names, lens, seqs, &columns);
	if (!rc) rc = rule_of(opts, &R);
	if (rc) return rc;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	try {
		t_alloc_s = 0;
		PileupBeside B(n_ref, R, names, lens, columns, seqs, nullptr, nullptr, command, out);
		rc = staged_alone(device, (const uint8_t *)records, n_bytes, n_ref, starts, n_starts, B, &out->stage_chunks, &out->count_s);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	out->alloc_s = t_alloc_s;  // (the arrays are freed by now)
	if (rc) urmapx_pileup_free(out);
	return rc;
}

}  // extern "C"
