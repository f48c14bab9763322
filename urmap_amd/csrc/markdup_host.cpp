// markdup_host.cpp -- duplicate marking without a device (urmapx_bam_sort_markdup_host; the rule is in include/urmapx.h "Duplicate
// marking").  Written apart from markdup.hip on purpose -- ends as tuples, std::stable_sort, a walk over the groups --, so that the two
// agreeing says something.
#include "bam_sort.h"

#include <algorithm>
#include <tuple>

namespace urx {
namespace bamsort {

namespace {
using End = std::tuple<uint32_t, int64_t, int>;  // refID as unsigned, u5, reverse
struct Rec {
	bool eligible = false;
	End end;
	uint32_t score = 0;
	int role = 0;  // 0: fragment, 1: first mate of a pair, 2: second mate
};

uint32_t flag_of(const uint8_t *r) { return load_u32(r + 16) >> 16; }

End end_of(const uint8_t *r) {
	const uint32_t l_name = r[12], n_cigar = load_u32(r + 16) & 0xFFFFu;
	const bool rev = flag_of(r) & 0x10u;
	const uint8_t *c = r + CORE + l_name;
	uint32_t first = n_cigar, last = n_cigar;  // the first and the last reference-consuming op
	int64_t span = 0;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t w = load_u32(c + 4u * k);
		if (!consumes_ref(w & 15u)) continue;
		if (first == n_cigar) first = k;
		last = k;
		span += w >> 4;
	}
	auto clips = [&](uint32_t a, uint32_t b) {
		int64_t s = 0;
		for (uint32_t k = a; k < b; ++k) {
			const uint32_t w = load_u32(c + 4u * k);
			if ((w & 15u) == 4u || (w & 15u) == 5u) s += w >> 4;
		}
		return s;
	};
	const int64_t pos = (int32_t)load_u32(r + 8);
	const int64_t u5 = rev ? pos + (span ? span : 1) - 1 + clips(last == n_cigar ? 0 : last + 1, n_cigar) : pos - clips(0, first);
	return End(load_u32(r + 4), u5, rev ? 1 : 0);
}
}  // namespace

int markdup_host(const uint8_t *rec, const std::vector<uint64_t> &offs, std::vector<uint8_t> &action, urmapx_markdup_stats *md) {
	const size_t n = offs.size() - 1;
	action.assign(n, MD_KEEP);
	std::vector<Rec> R(n);
	int bad = 0;
#pragma omp parallel for schedule(static) reduction(| : bad)
	for (int64_t s = 0; s < (int64_t)n; ++s) {
		const size_t i = (size_t)s;
		const uint8_t *r = rec + offs[i];
		if (flag_of(r) & (0x4u | 0x100u | 0x800u)) continue;
		const uint64_t len = offs[i + 1] - offs[i], l_seq = load_u32(r + 20);
		const uint64_t qual_at = (uint64_t)CORE + r[12] + 4ull * (load_u32(r + 16) & 0xFFFFu) + (l_seq + 1) / 2;
		if (qual_at + l_seq > len) { bad |= 1; continue; }
		uint64_t sum = 0;
		for (uint64_t k = 0; k < l_seq; ++k) {
			const uint8_t q = r[qual_at + k];
			if (q >= 15 && q != 0xFF) sum += q;
		}
		R[i].eligible = true;
		R[i].end = end_of(r);
		R[i].score = (uint32_t)std::min<uint64_t>(sum, MAX_SCORE);
		action[i] = MD_CLEAR;
	}
	if (bad) return URMAPX_E_FORMAT;

	// pairs, from the front
	std::vector<uint32_t> pairs, eligible;
	for (size_t i = 0; i < n; ++i) {
		if (!R[i].eligible) continue;
		eligible.push_back((uint32_t)i);
		if (R[i].role == 2 || i + 1 >= n || !R[i + 1].eligible) continue;
		const uint8_t *a = rec + offs[i], *b = rec + offs[i + 1];
		if ((flag_of(a) & 0xC1u) != 0x41u || (flag_of(b) & 0x81u) != 0x81u || a[12] != b[12] || !std::equal(a + CORE, a + CORE + a[12], b + CORE)) continue;
		R[i].role = 1;
		R[i + 1].role = 2;
		pairs.push_back((uint32_t)i);
	}

	// rule 5: the pairs of one key; the best stays
	auto pair_key = [&](uint32_t v) { return std::make_pair(std::min(R[v].end, R[v + 1].end), std::max(R[v].end, R[v + 1].end)); };
	auto pair_score = [&](uint32_t v) { return (uint64_t)R[v].score + R[v + 1].score; };
	std::stable_sort(pairs.begin(), pairs.end(), [&](uint32_t x, uint32_t y) { return pair_key(x) < pair_key(y); });
	uint64_t pair_dups = 0;
	for (size_t a = 0; a < pairs.size();) {
		size_t b = a, keep = a;
		for (; b < pairs.size() && pair_key(pairs[b]) == pair_key(pairs[a]); ++b)
			if (pair_score(pairs[b]) > pair_score(pairs[keep])) keep = b;  // (the sort is stable: among equals the first in the input comes first)
		for (size_t k = a; k < b; ++k)
			if (k != keep) { action[pairs[k]] = action[pairs[k] + 1] = MD_SET; ++pair_dups; }
		a = b;
	}

	// rule 6: the eligible records of one end; their fragments
	std::stable_sort(eligible.begin(), eligible.end(), [&](uint32_t x, uint32_t y) { return R[x].end < R[y].end; });
	uint64_t frags = 0, frag_dups = 0;
	for (size_t a = 0; a < eligible.size();) {
		size_t b = a;
		bool has_pair = false;
		int64_t keep = -1;
		for (; b < eligible.size() && R[eligible[b]].end == R[eligible[a]].end; ++b) {
			const Rec &x = R[eligible[b]];
			if (x.role) has_pair = true;
			else if (keep < 0 || x.score > R[eligible[(size_t)keep]].score) keep = (int64_t)b;
		}
		for (size_t k = a; k < b; ++k) {
			if (R[eligible[k]].role) continue;
			++frags;
			if (has_pair || (int64_t)k != keep) { action[eligible[k]] = MD_SET; ++frag_dups; }
		}
		a = b;
	}
	md->pairs_examined = pairs.size();
	md->pairs_duplicate = pair_dups;
	md->fragments_examined = frags;
	md->fragments_duplicate = frag_dups;
	return URMAPX_OK;
}

}  // namespace bamsort
}  // namespace urx
