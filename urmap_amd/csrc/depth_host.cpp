// depth_host.cpp -- per-base depth of BAM records without a device (urmapx_bam_depth_host; the rule is in include/urmapx.h "Depth"),
// and the host arithmetic the device version shares: the checks of the arguments and the sums of device bytes (depth.h).  Written
// apart from depth.hip on purpose -- one difference array, one running sum, std::to_string --, so that the two agreeing says something.
#include "depth.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

namespace urx {
namespace depth {

uint32_t text_runs() {
	const char *e = getenv("URMAPX_TEST_DEPTH_SLICE");
	const long long v = e ? atoll(e) : 0;
	return v >= 1 && v <= (long long)TEXT_RUNS ? (uint32_t)v : TEXT_RUNS;
}

int check_refs(uint32_t n_ref, const char *const *names, const uint32_t *lens, uint64_t *entries) {
	if (n_ref && (!names || !lens)) return URMAPX_E_ARG;
	uint64_t columns = 0;
	for (uint32_t r = 0; r < n_ref; ++r) {
		if (!names[r]) return URMAPX_E_ARG;
		const size_t l = strlen(names[r]);
		if (l < 1 || l > MAX_NAME) return URMAPX_E_ARG;
		columns += lens[r];
	}
	*entries = entries_of(columns, n_ref);
	return URMAPX_OK;
}

int scan_for_depth(const uint8_t *rec, size_t n_bytes, uint32_t n_ref, const uint64_t *starts, size_t n_starts, std::vector<uint64_t> &offs) {
	uint32_t max_pos = 0;
	const int rc = bamsort::scan_records(rec, n_bytes, n_ref, starts, n_starts, offs, max_pos);
	if (rc != URMAPX_E_FORMAT || n_bytes / bamsort::CORE < 0x7FFFFFFFu) return rc;
	// enough bytes for 2^31 records: is it their number the walk refused?
	uint64_t at = 0, n = 0;
	while (n_bytes - at >= bamsort::CORE && n < 0x7FFFFFFFu) {
		const uint64_t len = (uint64_t)bamsort::load_u32(rec + at) + 4u;
		if (len < bamsort::CORE || len > n_bytes - at) return rc;
		at += len;
		++n;
	}
	return n >= 0x7FFFFFFFu ? URMAPX_E_ARG : rc;
}

int depth_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
               uint32_t min_mapq, urmapx_depth_result *out) {
	using Clock = std::chrono::steady_clock;
	auto since = [](Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); };
	const size_t n = offs.size() - 1;
	out->records = n;
	out->n_ref = n_ref;
	out->refs = (urmapx_depth_summary *)calloc(n_ref ? n_ref : 1, sizeof(urmapx_depth_summary));
	if (!out->refs) return URMAPX_E_NOMEM;

	auto t = Clock::now();
	std::vector<uint64_t> first((size_t)n_ref + 1, 0);  // reference r's entries begin at first[r]: l_ref of them and one for ends beyond
	for (uint32_t r = 0; r < n_ref; ++r) first[r + 1] = first[r] + lens[r] + 1u;
	std::vector<int32_t> diff((size_t)first[n_ref], 0);
	for (size_t i = 0; i < n; ++i) {
		const uint8_t *r = rec + offs[i];
		const int32_t ref_id = (int32_t)bamsort::load_u32(r + 4), pos = (int32_t)bamsort::load_u32(r + 8);
		uint32_t flag = bamsort::load_u32(r + 16) >> 16;
		if (action && action[i] == bamsort::MD_SET) flag |= 0x400u;
		if (action && action[i] == bamsort::MD_CLEAR) flag &= ~0x400u;
		const uint32_t mapq = r[13];
		if (ref_id < 0 || (uint32_t)ref_id >= n_ref || pos < 0 || (flag & 0x704u) || mapq < min_mapq) continue;
		urmapx_depth_summary &S = out->refs[ref_id];
		++S.reads;
		S.mapq_sum += mapq;
		const uint32_t l_name = r[12], n_cigar = bamsort::load_u32(r + 16) & 0xFFFFu;
		if ((uint64_t)bamsort::CORE + l_name + 4ull * n_cigar > offs[i + 1] - offs[i]) continue;
		const int64_t l_ref = lens[ref_id];
		int64_t c = pos;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t w = bamsort::load_u32(r + bamsort::CORE + l_name + 4u * k), op = w & 15u;
			const int64_t len = w >> 4;
			if (op == 0u || op == 7u || op == 8u) {
				const int64_t beg = c < l_ref ? c : l_ref, end = c + len < l_ref ? c + len : l_ref;
				++diff[(size_t)(first[ref_id] + (uint64_t)beg)];
				--diff[(size_t)(first[ref_id] + (uint64_t)end)];
				c += len;
			} else if (op == 2u || op == 3u)
				c += len;
		}
	}
	out->count_s = since(t);

	t = Clock::now();
	std::string text;
	for (uint32_t r = 0; r < n_ref; ++r) {
		urmapx_depth_summary &S = out->refs[r];
		int64_t d = 0, run_d = 0;
		uint32_t run_beg = 0;
		auto line = [&](uint32_t end) {
			text += names[r];
			text += '\t'; text += std::to_string(run_beg);
			text += '\t'; text += std::to_string(end);
			text += '\t'; text += std::to_string(run_d);
			text += '\n';
			++out->runs;
		};
		for (uint32_t x = 0; x < lens[r]; ++x) {
			d += diff[(size_t)(first[r] + x)];
			if (x == 0) run_d = d;
			else if (d != run_d) { line(x); run_beg = x; run_d = d; }
			if (d > 0) { ++S.covered; S.bases += (uint64_t)d; }
		}
		if (lens[r]) line(lens[r]);
	}
	out->scan_s = since(t);
	t = Clock::now();
	out->text = (char *)malloc(text.size() ? text.size() : 1);
	if (!out->text) return URMAPX_E_NOMEM;
	memcpy(out->text, text.data(), text.size());
	out->text_bytes = text.size();
	out->format_s = since(t);
	return URMAPX_OK;
}

}  // namespace depth
}  // namespace urx

using namespace urx::depth;

extern "C" {

void urmapx_depth_free(urmapx_depth_result *R) {
	if (!R) return;
	free(R->text);
	free(R->refs);
	R->text = nullptr;
	R->refs = nullptr;
	R->text_bytes = 0;
	R->runs = 0;
	R->n_ref = 0;
}

uint64_t urmapx_bam_depth_resident_bytes(uint64_t total_columns, uint32_t n_ref) {
	return resident_bytes(entries_of(total_columns, n_ref), n_ref, text_runs());
}

uint64_t urmapx_bam_depth_device_bytes(uint64_t total_columns, uint32_t n_ref, uint64_t n_records) {
	return standalone_bytes(entries_of(total_columns, n_ref), n_ref, text_runs(), n_records, urx::bamsort::DEFAULT_STAGE);
}

int urmapx_bam_depth_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint64_t *starts,
                          size_t n_starts, const urmapx_depth_opts *opts, urmapx_depth_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t entries = 0;
	int rc = check_refs(n_ref, names, lens, &entries);
	if (rc) return rc;
	try {
		std::vector<uint64_t> offs;
		rc = scan_for_depth((const uint8_t *)records, n_bytes, n_ref, starts, n_starts, offs);
		if (!rc) rc = depth_host((const uint8_t *)records, offs, nullptr, n_ref, names, lens, opts ? opts->min_mapq : 0u, out);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	if (rc) urmapx_depth_free(out);
	return rc;
}

}  // extern "C"
