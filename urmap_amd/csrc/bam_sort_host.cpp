// bam_sort_host.cpp -- the coordinate sort of BAM records without a device (urmapx_bam_sort_host), and what it shares with the
// device sort of bam_sort.hip: the walk along the block_size chain, the members' table, the .bai writer.  See include/urmapx.h
// "Sorted BAM output" for the contract and bam_sort.h for the pieces.
#include "bam_sort.h"
#include "depth.h"
#include "pileup.h"
#include "stats.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>

namespace urx {
namespace bamsort {

namespace {
// the chain from `at` to exactly `stop`
int walk(const uint8_t *rec, uint64_t at, uint64_t stop, uint32_t n_ref, std::vector<uint64_t> &offs, uint32_t &max_pos) {
	const uint64_t n_bytes = stop;
	max_pos = 0;
	while (at < n_bytes) {
		if (n_bytes - at < CORE) return URMAPX_E_FORMAT;
		const uint8_t *r = rec + at;
		const uint64_t len = (uint64_t)load_u32(r) + 4u;
		const uint32_t ref_id = load_u32(r + 4), pos = load_u32(r + 8);
		const uint32_t l_name = load_u32(r + 12) & 0xFFu, n_cigar = load_u32(r + 16) & 0xFFFFu;
		if (len > n_bytes - at || (uint64_t)CORE + l_name + 4ull * n_cigar > len) return URMAPX_E_FORMAT;
		if (ref_id != 0xFFFFFFFFu && (ref_id >= n_ref || pos == 0xFFFFFFFFu)) return URMAPX_E_FORMAT;
		if (pos != 0xFFFFFFFFu) {
			if (pos >> 31) return URMAPX_E_FORMAT;
			max_pos = std::max(max_pos, pos);
		}
		if (offs.size() >= 0x7FFFFFFFu) return URMAPX_E_FORMAT;  // record numbers are 32 bits
		offs.push_back(at);
		at += len;
	}
	return URMAPX_OK;
}
}  // namespace

int scan_records(const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, std::vector<uint64_t> &offs, uint32_t &max_pos) {
	offs.clear();
	max_pos = 0;
	std::vector<uint64_t> cut{0};  // piece p is [cut[p], cut[p + 1])
	for (size_t k = 0; k < n_starts; ++k) {
		if (starts[k] < cut.back() || starts[k] > n_bytes) return URMAPX_E_FORMAT;
		if (starts[k] > cut.back()) cut.push_back(starts[k]);
	}
	if (cut.back() < n_bytes) cut.push_back(n_bytes);
	const int64_t P = (int64_t)cut.size() - 1;
	std::vector<std::vector<uint64_t>> part((size_t)P);
	std::vector<uint32_t> top((size_t)P, 0);
	std::vector<int> rcs((size_t)P, 0);
#pragma omp parallel for schedule(dynamic, 1) if (P > 1)
	for (int64_t p = 0; p < P; ++p) {
		part[(size_t)p].reserve((size_t)((cut[(size_t)p + 1] - cut[(size_t)p]) / 200));
		rcs[(size_t)p] = walk(rec, cut[(size_t)p], cut[(size_t)p + 1], n_ref, part[(size_t)p], top[(size_t)p]);
	}
	size_t n = 0;
	for (int64_t p = 0; p < P; ++p) {
		if (rcs[(size_t)p]) return rcs[(size_t)p];
		n += part[(size_t)p].size();
		max_pos = std::max(max_pos, top[(size_t)p]);
	}
	if (n >= 0x7FFFFFFFu) return URMAPX_E_FORMAT;
	offs.resize(n + 1);
	std::vector<size_t> first((size_t)P + 1, 0);
	for (int64_t p = 0; p < P; ++p) first[(size_t)p + 1] = first[(size_t)p] + part[(size_t)p].size();
#pragma omp parallel for schedule(dynamic, 1) if (P > 1)
	for (int64_t p = 0; p < P; ++p)
		if (!part[(size_t)p].empty()) memcpy(&offs[first[(size_t)p]], part[(size_t)p].data(), part[(size_t)p].size() * sizeof(uint64_t));
	offs[n] = n_bytes;
	return URMAPX_OK;
}

bool member_table(const uint8_t *z, size_t n, uint64_t in_front, std::vector<uint64_t> &coffs) {
	coffs.clear();
	size_t at = 0;
	while (at < n) {
		// 18 bytes of header, the 'BC' field with BSIZE = the member's size - 1 at 16 (urmapx.h "BGZF output")
		if (n - at < 28 || z[at] != 0x1f || z[at + 1] != 0x8b || z[at + 12] != 'B' || z[at + 13] != 'C') return false;
		const size_t size = ((size_t)z[at + 16] | (size_t)z[at + 17] << 8) + 1u;
		if (size < 26 || size > n - at) return false;
		coffs.push_back(in_front + at);
		at += size;
	}
	coffs.push_back(in_front + at);
	return true;
}

namespace {
void put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
void put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
}  // namespace

std::vector<uint8_t> write_bai(const IndexArrays &X, uint32_t n_ref, const std::vector<uint64_t> &coffs) {
	auto voff = [&](uint64_t u) {
		const uint64_t m = u / MEMBER;
		return (m < coffs.size() ? coffs[(size_t)m] : coffs.back()) << 16 | u % MEMBER;
	};
	std::vector<uint8_t> o;
	o.reserve(16 + 24 * X.chunks.size() + 8 * X.lin.size() + 64 * (size_t)n_ref);
	o.insert(o.end(), {'B', 'A', 'I', 1});
	put32(o, n_ref);
	size_t c = 0;
	for (uint32_t r = 0; r < n_ref; ++r) {
		const RefExtent &E = X.refs[r];
		const bool any = E.n_mapped + E.n_unmapped != 0;
		const size_t c0 = c;
		uint32_t n_bin = 0;
		for (; c < X.chunks.size() && X.chunks[c].ref == r; ++c)
			if (c == c0 || X.chunks[c].bin != X.chunks[c - 1].bin) ++n_bin;
		put32(o, n_bin + (any ? 1u : 0u));
		for (size_t a = c0; a < c;) {
			size_t b = a;
			while (b < c && X.chunks[b].bin == X.chunks[a].bin) ++b;
			put32(o, X.chunks[a].bin);
			put32(o, (uint32_t)(b - a));
			for (; a < b; ++a) { put64(o, voff(X.chunks[a].beg)); put64(o, voff(X.chunks[a].end)); }
		}
		if (any) {
			put32(o, PSEUDO_BIN);
			put32(o, 2);
			put64(o, voff(E.beg)); put64(o, voff(E.end));
			put64(o, E.n_mapped); put64(o, E.n_unmapped);
		}
		const uint64_t w0 = X.win_base[r], w1 = X.win_base[r + 1];
		put32(o, (uint32_t)(w1 - w0));
		const size_t at = o.size();
		o.resize(at + 8 * (size_t)(w1 - w0));
		uint64_t next = 0;  // (the last window of a reference is never empty: the windows end behind the last record)
		for (uint64_t w = w1; w-- > w0;) {
			if (X.lin[(size_t)w] != NONE) next = voff(X.lin[(size_t)w]);
			for (int k = 0; k < 8; ++k) o[at + 8 * (size_t)(w - w0) + (size_t)k] = (uint8_t)(next >> (8 * k));
		}
	}
	put64(o, X.n_no_coor);
	return o;
}

int finish_result(urmapx_bam_sort_result *out, uint8_t *bgzf, size_t bgzf_bytes, uint64_t stream_bytes, uint64_t in_front,
                  const IndexArrays &X, uint32_t n_ref) {
	out->bgzf = bgzf;
	out->bgzf_bytes = bgzf_bytes;
	out->stream_bytes = stream_bytes;
	std::vector<uint64_t> coffs;
	if (!member_table(bgzf, bgzf_bytes, in_front, coffs) || coffs.size() != (size_t)((stream_bytes + MEMBER - 1) / MEMBER) + 1u) return URMAPX_E_FORMAT;
	try {
		const std::vector<uint8_t> bai = write_bai(X, n_ref, coffs);
		out->bai = malloc(bai.size());
		if (!out->bai) return URMAPX_E_NOMEM;
		memcpy(out->bai, bai.data(), bai.size());
		out->bai_bytes = bai.size();
	} catch (const std::bad_alloc &) {
		return URMAPX_E_NOMEM;
	}
	return URMAPX_OK;
}

// ---- the device sort's plan: host arithmetic, shared with bam_sort.hip ----
namespace {
uint64_t env_number(const char *name, uint64_t most) {
	const char *e = getenv(name);
	const long long v = e ? atoll(e) : 0;
	return v >= 1 && (uint64_t)v <= most ? (uint64_t)v : 0;
}
}  // namespace
uint32_t slice_members() {
	const uint64_t v = env_number("URMAPX_TEST_SORT_SLICE", DEFAULT_SLICE);
	return v ? (uint32_t)v : DEFAULT_SLICE;
}
uint64_t test_partition_slices() { return env_number("URMAPX_TEST_SORT_PARTITION", (uint64_t)1 << 32); }
uint64_t test_stage_bytes() { return env_number("URMAPX_TEST_SORT_STAGE", (uint64_t)1 << 40); }

size_t slice_scratch_bytes(size_t slice_bytes) {
	return slice_bytes + urmapx_bgzf_bound(slice_bytes) + slice_bytes + slice_bytes / 64 + ((size_t)1024 * 255 << 10);
}

uint64_t external_device_bytes(size_t n_bytes, uint64_t n_records, bool markdup, uint64_t stage_bytes, uint64_t partition_bytes) {
	const size_t slice = (size_t)slice_members() * MEMBER, slice_cap = slice < n_bytes ? slice : n_bytes;
	const uint64_t per_record = SORT_PER_RECORD + (markdup ? MARKDUP_PER_RECORD + ACTION_PER_RECORD : 0u);
	// (a partition is not larger than the stream; the slice itself lies inside it: slice_scratch_bytes counts it, so it goes off again)
	const uint64_t part = partition_bytes < n_bytes ? partition_bytes : (uint64_t)n_bytes;
	return per_record * n_records + 2u * stage_bytes + part + (slice_scratch_bytes(slice_cap) - slice_cap) + SORT_SLACK + (markdup ? 4096u : 0u);
}

uint64_t default_stage_bytes(size_t n_bytes) {
	if (const uint64_t t = test_stage_bytes()) return t;
	const uint64_t cap = (uint64_t)n_bytes / 16u;  // (small inputs plan sensibly: two buffers are an eighth of them at the most)
	return DEFAULT_STAGE < cap ? DEFAULT_STAGE : cap;
}

int plan_with_stage(size_t n_bytes, uint64_t n_records, bool markdup, uint64_t budget, uint64_t stage_bytes, urmapx_bam_sort_plan *plan) {
	memset(plan, 0, sizeof *plan);
	const uint64_t forced = test_partition_slices();
	const uint64_t in_core = markdup ? urmapx_bam_sort_markdup_device_bytes(n_bytes, n_records) : urmapx_bam_sort_device_bytes(n_bytes, n_records);
	if (!forced && in_core <= budget) {
		plan->device_bytes = in_core;
		return URMAPX_OK;
	}
	const uint64_t slice = (uint64_t)slice_members() * MEMBER;
	const uint64_t whole = ((uint64_t)n_bytes + slice - 1) / slice;  // slices of the whole stream: a partition is never larger
	const uint64_t least = whole ? 1u : 0u;
	const uint64_t fixed = external_device_bytes(n_bytes, n_records, markdup, stage_bytes, 0);
	plan->external = 1;
	plan->stage_bytes = stage_bytes;
	// the most slices that fit: all of them where the whole stream does (the last slice may be a short one), else whole slices only
	uint64_t slices = forced ? forced : budget >= fixed + n_bytes ? whole : budget > fixed ? (budget - fixed) / slice : 0u;
	if (slices > whole) slices = whole;
	if (slices < least) {
		plan->device_bytes = external_device_bytes(n_bytes, n_records, markdup, stage_bytes, slice);
		return URMAPX_E_NOMEM;
	}
	plan->partition_bytes = slices * slice;
	plan->partitions = slices ? ((uint64_t)n_bytes + plan->partition_bytes - 1) / plan->partition_bytes : 0u;
	plan->device_bytes = external_device_bytes(n_bytes, n_records, markdup, stage_bytes, plan->partition_bytes);
	return URMAPX_OK;
}

}  // namespace bamsort
}  // namespace urx

using namespace urx::bamsort;

namespace {
using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

// a call once the marking has decided: the records as they came, their starts, and what becomes of every record's bit 0x400 (null
// without marking).  What it returns ends the sort if not 0 (urmapx_bam_sort_with_host takes the depth, the statistics and the pileup there)
using AfterMark = std::function<int(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action)>;

int sort_host(const uint8_t *rec, size_t n_bytes, uint32_t n_ref, uint64_t in_front, const uint64_t *starts, size_t n_starts, urmapx_markdup_stats *md,
              urmapx_bam_sort_result *out, const AfterMark *hook) {
	auto t = Clock::now();
	std::vector<uint64_t> offs;
	uint32_t max_pos = 0;
	int rc = scan_records(rec, n_bytes, n_ref, starts, n_starts, offs, max_pos);
	if (rc) return rc;
	out->scan_s = since(t);
	const size_t n = offs.size() - 1;
	out->records = n;
	const KeyLayout K = key_layout(n_ref, max_pos);

	t = Clock::now();
	std::vector<uint64_t> key(n);
	std::vector<uint32_t> perm(n);
	for (size_t i = 0; i < n; ++i) {
		key[i] = K.key(load_u32(rec + offs[i] + 4), load_u32(rec + offs[i] + 8));
		perm[i] = (uint32_t)i;
	}
	std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
	out->sort_s = since(t);

	// markdup: what becomes of every record's bit 0x400, applied to the copy below (the caller's records stay as they are)
	std::vector<uint8_t> action;
	if (md) {
		t = Clock::now();
		if ((rc = markdup_host(rec, offs, action, md))) return rc;
		md->markdup_s = since(t);
	}
	if (hook && (rc = (*hook)(rec, offs, md ? action.data() : nullptr))) return rc;

	t = Clock::now();
	std::vector<uint8_t> stream(n_bytes);
	std::vector<uint64_t> dst(n + 1);
	uint64_t at = 0;
	for (size_t k = 0; k < n; ++k) {
		const uint64_t a = offs[perm[k]], len = offs[perm[k] + 1] - a;
		dst[k] = at;
		if (len) memcpy(stream.data() + at, rec + a, (size_t)len);
		if (md && action[perm[k]] == MD_SET) stream[(size_t)at + FLAG_BYTE] |= FLAG_DUP_BIT;
		else if (md && action[perm[k]] == MD_CLEAR) stream[(size_t)at + FLAG_BYTE] &= (uint8_t)~FLAG_DUP_BIT;
		at += len;
	}
	dst[n] = at;
	out->gather_s = since(t);

	t = Clock::now();
	IndexArrays X;
	X.refs.assign(n_ref, RefExtent());
	X.win_base.assign((size_t)n_ref + 1, 0);
	std::vector<uint64_t> max_end(n_ref, 0), end_of(n);
	std::vector<uint32_t> bin_of(n), placed;
	for (size_t k = 0; k < n; ++k) {
		const uint32_t r = K.ref_of(key[perm[k]]);
		if (r == n_ref) { ++X.n_no_coor; continue; }
		const uint8_t *p = rec + offs[perm[k]];
		const uint64_t beg = K.pos_of(key[perm[k]]), end = ref_end(p, (uint32_t)(dst[k + 1] - dst[k]), beg);
		RefExtent &E = X.refs[r];
		if (E.n_mapped + E.n_unmapped == 0) E.beg = dst[k];
		E.end = dst[k + 1];
		if (load_u32(p + 16) >> 16 & 4u) ++E.n_unmapped; else ++E.n_mapped;
		if (!indexed(beg)) continue;  // (counted in the pseudo-bin, lying between its offsets; no chunk, no window)
		end_of[k] = index_end(end);
		max_end[r] = std::max(max_end[r], end_of[k]);
		bin_of[k] = reg2bin(beg, end_of[k]);
		placed.push_back((uint32_t)k);
	}
	for (uint32_t r = 0; r < n_ref; ++r) X.win_base[r + 1] = X.win_base[r] + (max_end[r] ? ((max_end[r] - 1) >> WINDOW_SHIFT) + 1 : 0);
	X.lin.assign((size_t)X.win_base[n_ref], NONE);
	for (uint32_t k : placed) {
		const uint32_t r = K.ref_of(key[perm[k]]);
		for (uint64_t w = K.pos_of(key[perm[k]]) >> WINDOW_SHIFT; w <= (end_of[k] - 1) >> WINDOW_SHIFT; ++w) {
			uint64_t &v = X.lin[(size_t)(X.win_base[r] + w)];
			if (dst[k] < v) v = dst[k];
		}
	}
	auto ref_bin = [&](uint32_t k) { return (uint64_t)K.ref_of(key[perm[k]]) << 32 | bin_of[k]; };
	std::stable_sort(placed.begin(), placed.end(), [&](uint32_t a, uint32_t b) { return ref_bin(a) < ref_bin(b); });
	for (size_t j = 0; j < placed.size(); ++j) {
		const uint32_t k = placed[j];
		if (j && ref_bin(placed[j - 1]) == ref_bin(k) && placed[j - 1] + 1 == k) X.chunks.back().end = dst[k + 1];
		else X.chunks.push_back(Chunk{K.ref_of(key[perm[k]]), bin_of[k], dst[k], dst[k + 1]});
	}
	out->no_coor = X.n_no_coor;
	out->index_s = since(t);

	t = Clock::now();
	const size_t cap = urmapx_bgzf_bound(n_bytes);
	uint8_t *z = (uint8_t *)malloc(cap ? cap : 1);
	if (!z) return URMAPX_E_NOMEM;
	size_t used = 0;
	rc = urmapx_bgzf_compress_host(stream.data(), n_bytes, z, cap, &used, 0);
	out->deflate_s = since(t);
	if (rc) { free(z); return rc; }
	t = Clock::now();
	rc = finish_result(out, z, used, n_bytes, in_front, X, n_ref);
	out->index_s += since(t);
	return rc;
}
}  // namespace

extern "C" {

static int sort_host_entry(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts, size_t n_starts,
                           urmapx_markdup_stats *md, urmapx_bam_sort_result *out, const AfterMark *hook = nullptr) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	if (md) memset(md, 0, sizeof *md);
	int rc;
	try {
		rc = sort_host((const uint8_t *)records, n_bytes, n_ref, bytes_in_front, starts, n_starts, md, out, hook);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	if (rc) urmapx_bam_sort_free(out);
	return rc;
}

int urmapx_bam_sort_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts, size_t n_starts,
                         urmapx_bam_sort_result *out) {
	return sort_host_entry(records, n_bytes, n_ref, bytes_in_front, starts, n_starts, nullptr, out);
}

int urmapx_bam_sort_markdup_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts,
                                 size_t n_starts, urmapx_markdup_stats *md, urmapx_bam_sort_result *out) {
	if (!md) return URMAPX_E_ARG;
	return sort_host_entry(records, n_bytes, n_ref, bytes_in_front, starts, n_starts, md, out);
}

int urmapx_bam_sort_plan_for(size_t n_bytes, uint64_t n_records, int markdup, uint64_t budget_bytes, urmapx_bam_sort_plan *plan) {
	if (!plan) return URMAPX_E_ARG;
	return plan_with_stage(n_bytes, n_records, markdup != 0, budget_bytes, default_stage_bytes(n_bytes), plan);
}

int urmapx_bam_sort_with_host(const void *records, size_t n_bytes, uint32_t n_ref, uint64_t bytes_in_front, const uint64_t *starts, size_t n_starts,
                              const urmapx_bam_sort_extras *extras, urmapx_bam_sort_result *out) {
	const urmapx_bam_sort_extras none{};
	const urmapx_bam_sort_extras &E = extras ? *extras : none;
	if (!E.depth && !E.stats && !E.pileup) {
		return E.md ? urmapx_bam_sort_markdup_host(records, n_bytes, n_ref, bytes_in_front, starts, n_starts, E.md, out)
		            : urmapx_bam_sort_host(records, n_bytes, n_ref, bytes_in_front, starts, n_starts, out);
	}
	if (E.depth) memset(E.depth, 0, sizeof *E.depth);
	if (E.stats) memset(E.stats, 0, sizeof *E.stats);
	if (E.pileup) memset(E.pileup, 0, sizeof *E.pileup);
	uint64_t columns = 0;
	urx::pileup::Rule R;
	int rc = urx::depth::check_refs(n_ref, E.names, E.lens, &columns);
	if (!rc && E.pileup) rc = urx::pileup::rule_of(E.popts, &R);
	if (rc) return rc;
	try {
		std::vector<uint8_t> store;
		std::vector<const uint8_t *> ptrs;
		const uint8_t *const *seqs = E.seqs;
		if (E.pileup && !seqs) {
			if ((rc = urx::pileup::index_sequences(E.index, n_ref, E.lens, store, ptrs))) return rc;
			seqs = ptrs.data();
		}
		if (E.pileup && (rc = urx::pileup::check_input(n_ref, E.names, E.lens, seqs, &columns))) return rc;
		// the flags as written: the marking's decisions beside the records as they came (order matters to none of the three)
		const AfterMark hook = [&](const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action) -> int {
			if (offs.size() - 1 >= 0x7FFFFFFFu) return URMAPX_E_ARG;
			if (E.depth)
				if (const int r = urx::depth::depth_host(rec, offs, action, n_ref, E.names, E.lens, E.dopts ? E.dopts->min_mapq : 0u, E.depth)) return r;
			if (E.stats)
				if (const int r = urx::stats::stats_host(rec, offs, action, n_ref, E.names, E.lens, E.stats_command, E.stats)) return r;
			return E.pileup ? urx::pileup::pileup_host(rec, offs, action, n_ref, E.names, E.lens, seqs, R, E.pileup_command, E.pileup) : URMAPX_OK;
		};
		rc = sort_host_entry(records, n_bytes, n_ref, bytes_in_front, starts, n_starts, E.md, out, &hook);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	if (rc && E.depth) urmapx_depth_free(E.depth);
	if (rc && E.stats) urmapx_stats_free(E.stats);
	if (rc && E.pileup) urmapx_pileup_free(E.pileup);
	return rc;
}

void urmapx_bam_sort_free(urmapx_bam_sort_result *R) {
	if (!R) return;
	free(R->bgzf);
	free(R->bai);
	R->bgzf = R->bai = nullptr;
	R->bgzf_bytes = R->bai_bytes = 0;
}

}  // extern "C"
