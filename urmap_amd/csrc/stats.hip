// stats.hip -- alignment statistics of BAM records on the device (urmapx_bam_stats, and the statistics step of urmapx_bam_sort_with; the
// rule is in include/urmapx.h "Stats", the layout of the tables, the LDS sizes and the memory sum in stats.h, the host version and the
// formatter in stats_host.cpp).
//
//   stats_count_kernel   persistent workgroups of sixteen wavefronts, one workgroup a compute unit; a WAVEFRONT takes one record at a
//                        time.  Nine lanes load the core words, which become scalars.  The CIGAR is taken 64 ops at a time, a lane an
//                        op; the aux area is walked by the whole wavefront in step (a Z or H value is searched for its end 64 bytes at a
//                        time); SEQ and QUAL are walked 64 bases a step, lane = base, so the lanes of a step fall on 64 different cycle
//                        rows.  The hot low ends of the tables -- both quality tables and BC below L_CYCLES cycles, MQ, GC, IS, RL, ID
//                        and RF below their L_ caps -- are 32-bit counters in LDS; everything beyond goes to the 64-bit tables by
//                        atomicAdd.  The SN counters: lane k of a wavefront keeps counter k in a register over all its records (the
//                        sums over CIGAR ops and bases stay per lane and are added up once, at the end), then one 64-bit LDS atomic
//                        a counter and wavefront.  At the end the workgroup adds its LDS bins that are not zero to the tables: once
//                        per workgroup and launch.
//                        A 32-bit bin cannot wrap: a record adds at most LANE_OPS to a bin (one to every bin but ID's, where only the
//                        first LANE_OPS ops of a CIGAR count in LDS), and a launch has at most LAUNCH_RECORDS = 2^28 records.
#include "stats_dev.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

#include "depth.h"

using namespace urx::bamsort;
using namespace urx::stats;

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

constexpr uint32_t SNT = urx::stats::NT;
constexpr uint32_t WAVES = SNT / 64;
// where the LDS copies begin, in 32-bit words
constexpr uint32_t S_Q = 0;                                  // [2][L_CYCLES][L_QROW]
constexpr uint32_t S_BC = S_Q + 2u * L_CYCLES * L_QROW;      // [L_CYCLES][BASES]
constexpr uint32_t S_MQ = S_BC + L_CYCLES * BASES;           // [256]
constexpr uint32_t S_GC = S_MQ + 256u;                       // [104]
constexpr uint32_t S_IS = S_GC + 104u;                       // [L_IS][3]
constexpr uint32_t S_RL = S_IS + 3u * L_IS;                  // [L_RL][2]
constexpr uint32_t S_ID = S_RL + 2u * L_RL;                  // [L_ID][2]
constexpr uint32_t S_RF = S_ID + 2u * L_ID;                  // [L_RF][3]
static_assert(S_RF + 3u * L_RF == LDS_WORDS, "the LDS layout and its size");
constexpr uint32_t NO_BIN32 = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t lane_word(uint32_t v, uint32_t from) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)from); }
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
	for (int s = 32; s; s >>= 1) v += (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64);
	return v;
}
__device__ __forceinline__ uint32_t elem_width(uint32_t t) {
	return t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' || t == 'f' ? 4u : 0u;
}

// The NM of the aux area [a, e) (rule 5); every lane of the wavefront walks in step and gets the same answer
__device__ __forceinline__ bool find_nm(const uint8_t *a, const uint8_t *e, uint32_t lane, uint64_t &nm) {
	while (e - a >= 3) {
		const bool is_nm = a[0] == 'N' && a[1] == 'M';
		const uint32_t t = a[2];
		a += 3;
		const uint64_t left = (uint64_t)(e - a);
		uint64_t size = t == 'A' ? 1u : elem_width(t);
		if (t == 'Z' || t == 'H') {
			size = 0;
			for (uint64_t p = 0; p < left && !size; p += 64u) {
				const unsigned long long m = __ballot(p + lane < left && a[p + lane] == 0);
				if (m) size = p + (uint64_t)__ffsll((long long)m);
			}
			if (!size) return false;
		} else if (t == 'B') {
			if (left < 5) return false;
			const uint32_t w = elem_width(a[0]);
			if (!w) return false;
			size = 5u + (uint64_t)load_u32(a + 1) * w;
		} else if (!size)
			return false;
		if (size > left) return false;
		if (is_nm && elem_width(t) && t != 'f') {
			const uint32_t raw = size == 1 ? a[0] : size == 2 ? (uint32_t)a[0] | (uint32_t)a[1] << 8 : load_u32(a);
			const bool negative = (t == 'c' && raw >> 7) || (t == 's' && raw >> 15) || (t == 'i' && raw >> 31);
			nm = negative ? 0u : raw;
			return true;
		}
		a += size;
	}
	return false;
}

__global__ __launch_bounds__(SNT) void stats_count_kernel(const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action,
                                                          uint32_t n_ref, unsigned long long *tab) {
	__shared__ uint32_t s_w[LDS_WORDS];
	__shared__ unsigned long long s_sn[SN_N];
	for (uint32_t x = threadIdx.x; x < LDS_WORDS; x += SNT) s_w[x] = 0;
	if (threadIdx.x < SN_N) s_sn[threadIdx.x] = 0;
	__syncthreads();

	const uint32_t lane = threadIdx.x & 63u, wave = uni(threadIdx.x >> 6), n = i1 - i0;
	uint64_t acc = 0;  // SN counter `lane` of this wavefront's records
	uint64_t p_aligned = 0, p_soft = 0, p_ins_b = 0, p_del_b = 0, p_ins = 0, p_del = 0, p_nm_bases = 0, p_qual = 0;  // this lane's share of the sums over ops and bases
	for (uint64_t k = (uint64_t)blockIdx.x * WAVES + wave; k < n; k += (uint64_t)gridDim.x * WAVES) {
		const uint64_t i = i0 + k, at = off[i], len = off[i + 1] - at;
		const uint8_t *r = rec + (at - base);
		const uint32_t hw = lane < 9u ? load_u32(r + 4u * lane) : 0u;
		const uint32_t ref = lane_word(hw, 1), w3 = lane_word(hw, 3), w4 = lane_word(hw, 4), next_ref = lane_word(hw, 6);
		uint32_t l_seq = lane_word(hw, 5), n_cigar = w4 & 0xFFFFu, flag = w4 >> 16;
		const int32_t tlen = (int32_t)lane_word(hw, 8);
		if (action) {
			const uint8_t a = action[i];
			if (a == MD_SET) flag |= 0x400u;
			else if (a == MD_CLEAR) flag &= ~0x400u;
		}
		flag = uni(flag);
		uint64_t ones = 1ull << SN_RECORDS;  // bit c: SN counter c takes one
		if (flag & 0x100u) ones |= 1ull << SN_SECONDARY;
		if (flag & 0x800u) ones |= 1ull << SN_SUPPLEMENTARY;
		if (flag & 0x900u) {
			acc += ones >> lane & 1u;
			continue;
		}
		const uint32_t l_name = w3 & 0xFFu, mapq = w3 >> 8 & 0xFFu;
		const uint8_t *cig = r + CORE + l_name, *const end = r + len, *aux = end;
		if ((uint64_t)CORE + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + l_seq > len) {
			l_seq = 0;
			n_cigar = 0;
		} else
			aux = cig + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + l_seq;
		const uint8_t *seq = cig + 4ull * n_cigar, *qual = seq + ((uint64_t)l_seq + 1u) / 2u;
		const bool paired = flag & 1u, mapped = !(flag & 4u), rev = flag & 0x10u, last = flag & 0x80u, dup = flag & 0x400u, mate_unmapped = flag & 8u;
		const bool has_qual = l_seq && qual[0] != 0xFFu;

		ones |= 1ull << SN_READS | 1ull << (last ? SN_LAST : SN_FIRST) | 1ull << (mapped ? SN_MAPPED : SN_UNMAPPED);
		if (paired) ones |= 1ull << SN_PAIRED;
		if (paired && mapped && (flag & 2u)) ones |= 1ull << SN_PROPER;
		if (paired && mapped && !mate_unmapped) ones |= 1ull << SN_MAPPED_PAIRED | (next_ref != ref ? 1ull << SN_MATE_OTHER : 0ull);
		if (paired && mapped && mate_unmapped) ones |= 1ull << SN_SINGLETONS;
		if (mapped && rev) ones |= 1ull << SN_REVERSE;
		if (dup) ones |= 1ull << SN_DUP;
		if (flag & 0x200u) ones |= 1ull << SN_QCFAIL;
		if (mapped && mapq == 0) ones |= 1ull << SN_MQ0;
		if (l_seq && !has_qual) ones |= 1ull << SN_NOQUAL;
		uint64_t lens = 1ull << SN_TOTAL_LEN;  // bit c: SN counter c takes l_seq
		if (mapped) lens |= 1ull << SN_BASES_MAPPED;
		if (dup) lens |= 1ull << SN_BASES_DUP;
		if (has_qual) lens |= 1ull << SN_QUAL_BASES;

		// one bin each of RL, RF (two), MQ, IS and GC: a lane each, one LDS atomic for all; a bin beyond the LDS copy goes to the tables
		uint32_t bin = NO_BIN32;
		{
			const uint32_t rl = l_seq < RL_MAX ? l_seq : RL_MAX, side = last ? 1u : 0u;
			if (rl < L_RL) { if (lane == 0) bin = S_RL + 2u * rl + side; }
			else if (lane == 0) atomicAdd(tab + T_RL + 2ull * rl + side, 1ull);
			const uint32_t row = ref < n_ref ? ref : n_ref;
			if (row < L_RF) {
				if (lane == 1) bin = S_RF + 3u * row + (mapped ? 0u : 1u);
				if (lane == 2 && dup) bin = S_RF + 3u * row + 2u;
			} else if (lane == 0) {
				atomicAdd(tab + T_RF + 3ull * row + (mapped ? 0u : 1u), 1ull);
				if (dup) atomicAdd(tab + T_RF + 3ull * row + 2u, 1ull);
			}
			if (mapped && lane == 3) bin = S_MQ + mapq;
			if (mapped && paired && !mate_unmapped && next_ref == ref && tlen > 0) {
				const uint32_t size = (uint32_t)tlen < IS_MAX ? (uint32_t)tlen : IS_MAX;
				const bool mate_rev = flag & 0x20u;
				const uint32_t kind = !rev && mate_rev ? 0u : rev && !mate_rev ? 1u : 2u;
				if (size < L_IS) { if (lane == 4) bin = S_IS + 3u * size + kind; }
				else if (lane == 0) atomicAdd(tab + T_IS + 3ull * size + kind, 1ull);
			}
		}

		uint64_t nm = 0;
		if (mapped) {
			uint64_t mine = 0;  // this lane's M, =, X and I lengths of this record
			for (uint32_t o0 = 0; o0 < n_cigar; o0 += 64u) {
				const uint32_t o = o0 + lane;
				if (o < n_cigar) {
					const uint32_t w = load_u32(cig + 4ull * o), op = w & 15u, L = w >> 4;
					if (op == 0u || op == 7u || op == 8u || op == 1u) mine += L;
					if (op == 4u) p_soft += L;
					if (op == 1u || op == 2u) {
						const uint32_t del = op == 2u ? 1u : 0u;
						if (del) p_del_b += L; else p_ins_b += L;
						if (L) {
							if (del) ++p_del; else ++p_ins;
							if (o < LANE_OPS && L < L_ID) atomicAdd(&s_w[S_ID + 2u * L + del], 1u);
							else atomicAdd(tab + T_ID + 2ull * (L < ID_MAX ? L : ID_MAX) + del, 1ull);
						}
					}
				}
			}
			p_aligned += mine;
			if (find_nm(aux, end, lane, nm)) {
				ones |= 1ull << SN_WITH_NM;
				p_nm_bases += mine;
			} else
				nm = 0;
		}

		// SEQ and QUAL: lane = base
		uint32_t gc = 0;
		const uint32_t qside = last ? 1u : 0u;
		for (uint64_t b0 = 0; b0 < l_seq; b0 += 64u) {
			const uint64_t b = b0 + lane;
			const bool in = b < l_seq;
			uint32_t code = 0;
			if (in) {
				code = b & 1u ? seq[b >> 1] & 15u : seq[b >> 1] >> 4;
				const uint64_t cyc = rev ? (uint64_t)l_seq - 1u - b : b;
				uint32_t cls = code == 1u ? 0u : code == 2u ? 1u : code == 4u ? 2u : code == 8u ? 3u : code == 15u ? 4u : 5u;
				if (rev && cls < 4u) cls = 3u - cls;
				if (cyc < L_CYCLES) atomicAdd(&s_w[S_BC + (uint32_t)cyc * BASES + cls], 1u);
				else atomicAdd(tab + T_BC + (uint64_t)BASES * (cyc < CYCLES ? cyc : CYCLES) + cls, 1ull);
				if (has_qual) {
					const uint32_t qb = qual[b], q = qb < QUALS - 1u ? qb : QUALS - 1u;
					p_qual += q;
					if (cyc < L_CYCLES) atomicAdd(&s_w[S_Q + (qside * L_CYCLES + (uint32_t)cyc) * L_QROW + q], 1u);
					else atomicAdd(tab + T_Q + (uint64_t)QUALS * ((uint64_t)qside * (CYCLES + 1u) + (cyc < CYCLES ? cyc : CYCLES)) + q, 1ull);
				}
			}
			gc += (uint32_t)__popcll(__ballot(in && (code == 2u || code == 4u)));
		}
		if (l_seq && lane == 5) bin = S_GC + (uint32_t)(100ull * gc / l_seq);
		if (bin != NO_BIN32) atomicAdd(&s_w[bin], 1u);

		acc += (ones >> lane & 1u) + (lens >> lane & 1u ? (uint64_t)l_seq : 0u);
		if (lane == SN_MISMATCHES) acc += nm;
		if (lane == SN_MAX_LEN && l_seq > acc) acc = l_seq;
	}

	// the sums the lanes kept apart; then a 64-bit LDS atomic per counter
	{
		const uint64_t sums[8] = {wave_sum64(p_aligned), wave_sum64(p_soft), wave_sum64(p_ins_b), wave_sum64(p_del_b),
		                          wave_sum64(p_ins),     wave_sum64(p_del),  wave_sum64(p_nm_bases), wave_sum64(p_qual)};
		const uint32_t to[8] = {SN_BASES_CIGAR, SN_SOFT, SN_BASES_INS, SN_BASES_DEL, SN_INS, SN_DEL, SN_NM_BASES, SN_QUAL_SUM};
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c)
			if (lane == to[c]) acc += sums[c];
		if (acc) {
			if (lane == SN_MAX_LEN) atomicMax(&s_sn[lane], (unsigned long long)acc);
			else atomicAdd(&s_sn[lane], (unsigned long long)acc);
		}
	}
	__syncthreads();

	// the workgroup's bins into the tables
	for (uint32_t x = threadIdx.x; x < LDS_WORDS; x += SNT) {
		const uint32_t v = s_w[x];
		if (!v) continue;
		uint64_t g;
		if (x < S_BC) {
			const uint32_t side = x / (L_CYCLES * L_QROW), in = x % (L_CYCLES * L_QROW), cyc = in / L_QROW, q = in % L_QROW;  // (q below QUALS: the pad is never counted in)
			g = T_Q + (uint64_t)QUALS * ((uint64_t)side * (CYCLES + 1u) + cyc) + q;
		} else if (x < S_MQ) g = T_BC + (x - S_BC);
		else if (x < S_GC) g = T_MQ + (x - S_MQ);
		else if (x < S_IS) g = T_GC + (x - S_GC);
		else if (x < S_RL) g = T_IS + (x - S_IS);
		else if (x < S_ID) g = T_RL + (x - S_RL);
		else if (x < S_RF) g = T_ID + (x - S_ID);
		else g = T_RF + (x - S_RF);  // (rows up to n_ref only were counted in)
		atomicAdd(tab + g, (unsigned long long)v);
	}
	if (threadIdx.x < SN_N) {
		const unsigned long long v = s_sn[threadIdx.x];
		if (v) {
			if (threadIdx.x == SN_MAX_LEN) atomicMax(tab + T_SN + threadIdx.x, v);
			else atomicAdd(tab + T_SN + threadIdx.x, v);
		}
	}
}

}  // namespace

namespace urx {
namespace stats {

int StatsOwn::begin(uint32_t n_ref_) {
	n_ref = n_ref_;
	int dev = 0, cus = 0;
	HIP_TRY(hipGetDevice(&dev));
	HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
	blocks = cus > 0 ? (uint32_t)cus : 1u;
	if (const uint32_t most = test_blocks()) blocks = std::min(blocks, most);
	if (const int rc = tab.alloc((size_t)table_words(n_ref))) return rc;
	HIP_TRY(hipMemset(tab.p, 0, (size_t)table_words(n_ref) * 8));
	return URMAPX_OK;
}

int stats_count(const StatsOwn &W, const uint8_t *rec, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) {
	for (uint64_t j0 = i0; j0 < i1; j0 += LAUNCH_RECORDS) {
		const uint32_t j1 = (uint32_t)std::min<uint64_t>(j0 + LAUNCH_RECORDS, i1);
		const uint32_t want = (j1 - (uint32_t)j0 + SNT / 64 - 1) / (SNT / 64);  // a wavefront a record
		hipLaunchKernelGGL(stats_count_kernel, dim3(std::min(W.blocks, want)), dim3(SNT), 0, stream, rec, base, off, (uint32_t)j0, j1, action, W.n_ref, W.tab.p);
	}
	return URMAPX_OK;
}

int stats_finish(StatsOwn &W, const char *const *names, const uint32_t *lens, const char *command, urmapx_stats_result *out) {
	const auto t = Clock::now();
	std::vector<uint64_t> tab((size_t)table_words(W.n_ref));
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpy(tab.data(), W.tab.p, tab.size() * 8, hipMemcpyDeviceToHost));
	const int rc = format_tables(tab.data(), W.n_ref, names, lens, command, out);
	out->format_s = since(t);
	return rc;
}

uint64_t StatsBeside::resident_bytes() const { return urx::stats::resident_bytes(n_ref); }
int StatsBeside::begin(uint32_t) { return W.begin(n_ref); }
int StatsBeside::count(const uint8_t *at, uint64_t base, const uint64_t *off, uint32_t i0, uint32_t i1, const uint8_t *action, hipStream_t stream) {
	return stats_count(W, at, base, off, i0, i1, action, stream);
}
int StatsBeside::finish() { return stats_finish(W, names, lens, command, out); }
void StatsBeside::free_result() { urmapx_stats_free(out); }

}  // namespace stats
}  // namespace urx

extern "C" {

int urmapx_bam_stats(int device, const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint64_t *starts,
                     size_t n_starts, const char *command, urmapx_stats_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t entries = 0;
	int rc = urx::depth::check_refs(n_ref, names, lens, &entries);
	if (rc) return rc;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) { (void)hipGetLastError(); return URMAPX_E_NODEVICE; }
	try {
		t_alloc_s = 0;
		StatsBeside B(n_ref, names, lens, command, out);
		rc = staged_alone(device, (const uint8_t *)records, n_bytes, n_ref, starts, n_starts, B, &out->stage_chunks, &out->count_s);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	out->alloc_s = t_alloc_s;  // (the arrays are freed by now)
	if (rc) urmapx_stats_free(out);
	return rc;
}

}  // extern "C"
