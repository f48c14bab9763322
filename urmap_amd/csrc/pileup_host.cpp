// pileup_host.cpp -- SNV candidate sites of BAM records without a device (urmapx_bam_pileup_host; the rule is in include/urmapx.h
// "Pileup"), and the host arithmetic the device version shares: the checks of the arguments, the test knobs, the sums of device bytes
// (pileup.h) and the one formatter of the text.  The walk is written apart from pileup.hip on purpose -- one record, one op, one base at
// a time on one thread --, so that the two agreeing says something.
#include "pileup.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "depth.h"
#include "stats.h"

namespace urx {
namespace pileup {

static long long env_number(const char *name) {
	const char *e = getenv(name);
	return e ? atoll(e) : 0;
}
uint32_t test_blocks() {
	const long long v = env_number("URMAPX_TEST_PILEUP_BLOCKS");
	return v >= 1 && v <= 65536 ? (uint32_t)v : 0u;
}
uint64_t segment_columns() {
	const long long v = env_number("URMAPX_TEST_PILEUP_SEGMENT");
	return v >= 1 && v <= (long long)SEGMENT ? ((uint64_t)v + NT - 1) / NT * NT : SEGMENT;
}
uint32_t slice_sites() {
	const long long v = env_number("URMAPX_TEST_PILEUP_SLICE");
	return v >= 1 && v <= (long long)SLICE_SITES ? (uint32_t)v : SLICE_SITES;
}

int rule_of(const urmapx_pileup_opts *opts, Rule *R) {
	*R = Rule();
	if (!opts) return URMAPX_OK;
	if (opts->min_mapq > 255u || opts->min_baseq > 255u || opts->min_alt == 0u || opts->min_pct > 100u) return URMAPX_E_ARG;
	R->min_mapq = opts->min_mapq; R->min_baseq = opts->min_baseq; R->min_alt = opts->min_alt; R->min_pct = opts->min_pct;
	return URMAPX_OK;
}

int check_input(uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint8_t *const *seqs, uint64_t *columns) {
	uint64_t entries = 0;
	if (const int rc = depth::check_refs(n_ref, names, lens, &entries)) return rc;
	*columns = entries - n_ref;
	if (n_ref && !seqs) return URMAPX_E_ARG;
	for (uint32_t r = 0; r < n_ref; ++r)
		if (lens[r] && !seqs[r]) return URMAPX_E_ARG;
	return URMAPX_OK;
}

int index_sequences(const urmapx_index *I, uint32_t n_ref, const uint32_t *lens, std::vector<uint8_t> &store, std::vector<const uint8_t *> &ptrs) {
	if (!I || urmapx_index_seq_count(I) != n_ref) return URMAPX_E_ARG;
	std::vector<uint64_t> at((size_t)n_ref), to((size_t)n_ref + 1, 0);
	for (uint32_t r = 0; r < n_ref; ++r) {
		if (urmapx_index_seq_length(I, r) != lens[r]) return URMAPX_E_ARG;
		at[r] = urmapx_index_seq_offset(I, r);
		to[r + 1] = to[r] + lens[r];
	}
	store.assign((size_t)to[n_ref] + 1, 0);
	if (const int rc = urmapx_index_fetch_spans(I, at.data(), lens, n_ref, store.data())) return rc;
	ptrs.resize(n_ref);
	for (uint32_t r = 0; r < n_ref; ++r) ptrs[r] = store.data() + to[r];
	return URMAPX_OK;
}

int format_sites(const Site *sites, size_t n_sites, uint32_t n_ref, const char *const *names, const uint32_t *lens, const Rule &R, const char *command,
                 urmapx_pileup_result *out) {
	std::string t = "##fileformat=VCFv4.2\n##source=urmap\n##urmapCommand=";
	t += command ? command : "";
	t += '\n';
	for (uint32_t r = 0; r < n_ref; ++r) {
		t += "##contig=<ID="; t += names[r]; t += ",length="; t += std::to_string(lens[r]); t += ">\n";
	}
	t += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Bases counted on the column\">\n"
	     "##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Bases counted per allele, the reference's first\">\n"
	     "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
	static const char LETTER[4] = {'A', 'C', 'G', 'T'};
	uint32_t r = 0;
	uint64_t first = 0;  // where reference r's columns begin
	out->sites = 0;
	out->alt_alleles = 0;
	for (size_t k = 0; k < n_sites; ++k) {
		const Site &S = sites[k];
		const uint64_t g = S.column & COLUMN_MASK;
		const uint32_t ref = (uint32_t)(S.column >> REF_SHIFT);
		while (r < n_ref && g >= first + lens[r]) first += lens[r++];
		if (r >= n_ref || g < first) return URMAPX_E_FORMAT;  // (not ascending, or beyond the last column)
		const uint64_t dp = (uint64_t)S.cnt[0] + S.cnt[1] + S.cnt[2] + S.cnt[3];
		uint32_t alt[3], n_alt = 0;
		for (uint32_t b = 0; b < 4u; ++b)
			if (b != ref && S.cnt[b] >= R.min_alt && (uint64_t)S.cnt[b] * 100u >= (uint64_t)R.min_pct * dp) alt[n_alt++] = b;
		if (!n_alt) return URMAPX_E_FORMAT;
		for (uint32_t i = 1; i < n_alt; ++i)  // by count descending; equal counts keep the order A C G T
			for (uint32_t j = i; j > 0 && S.cnt[alt[j]] > S.cnt[alt[j - 1]]; --j) std::swap(alt[j], alt[j - 1]);
		t += names[r]; t += '\t'; t += std::to_string(g - first + 1u); t += "\t.\t"; t += LETTER[ref]; t += '\t';
		for (uint32_t i = 0; i < n_alt; ++i) { if (i) t += ','; t += LETTER[alt[i]]; }
		t += "\t.\t.\tDP="; t += std::to_string(dp); t += ";AD="; t += std::to_string(S.cnt[ref]);
		for (uint32_t i = 0; i < n_alt; ++i) { t += ','; t += std::to_string(S.cnt[alt[i]]); }
		t += '\n';
		++out->sites;
		out->alt_alleles += n_alt;
	}
	out->text = (char *)malloc(t.size() ? t.size() : 1);
	if (!out->text) return URMAPX_E_NOMEM;
	memcpy(out->text, t.data(), t.size());
	out->text_bytes = t.size();
	return URMAPX_OK;
}

int pileup_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
                const uint8_t *const *seqs, const Rule &R, const char *command, urmapx_pileup_result *out) {
	using Clock = std::chrono::steady_clock;
	auto since = [](Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); };
	const size_t n = offs.size() - 1;
	auto t = Clock::now();
	std::vector<uint64_t> first((size_t)n_ref + 1, 0);
	for (uint32_t r = 0; r < n_ref; ++r) first[r + 1] = first[r] + lens[r];
	std::vector<uint32_t> cnt((size_t)first[n_ref] * 4u, 0);
	for (size_t i = 0; i < n; ++i) {
		const uint8_t *r = rec + offs[i];
		const uint64_t size = offs[i + 1] - offs[i];
		const int32_t ref_id = (int32_t)bamsort::load_u32(r + 4), pos = (int32_t)bamsort::load_u32(r + 8);
		uint32_t flag = bamsort::load_u32(r + 16) >> 16;
		if (action && action[i] == bamsort::MD_SET) flag |= 0x400u;
		if (action && action[i] == bamsort::MD_CLEAR) flag &= ~0x400u;
		if (ref_id < 0 || (uint32_t)ref_id >= n_ref || pos < 0 || (flag & 0x704u) || r[13] < R.min_mapq) continue;
		++out->records;
		const uint32_t l_name = r[12], n_cigar = bamsort::load_u32(r + 16) & 0xFFFFu;
		const uint64_t l_seq = bamsort::load_u32(r + 20);
		if ((uint64_t)bamsort::CORE + l_name + 4ull * n_cigar + (l_seq + 1u) / 2u + l_seq > size) continue;
		const uint8_t *cigar = r + bamsort::CORE + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + (l_seq + 1u) / 2u;
		const bool no_qual = l_seq && qual[0] == 0xFFu;
		const uint64_t l_ref = lens[ref_id];
		uint32_t *const C = cnt.data() + 4u * first[ref_id];
		uint64_t x = (uint64_t)pos, q = 0;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t w = bamsort::load_u32(cigar + 4ull * k), op = w & 15u;
			const uint64_t len = w >> 4;
			if (op == 0u || op == 7u || op == 8u) {
				for (uint64_t j = 0; j < len && x + j < l_ref && q + j < l_seq; ++j) {
					const uint64_t b = q + j;
					const uint32_t code = b % 2u ? seq[b / 2u] % 16u : seq[b / 2u] / 16u;
					if (code != 1u && code != 2u && code != 4u && code != 8u) continue;
					if (!no_qual && qual[b] < R.min_baseq) continue;
					++C[4u * (x + j) + (code == 1u ? 0 : code == 2u ? 1 : code == 4u ? 2 : 3)];
				}
				x += len; q += len;
			} else if (op == 1u || op == 4u)
				q += len;
			else if (op == 2u || op == 3u)
				x += len;
		}
	}
	out->count_s = since(t);

	t = Clock::now();
	std::vector<Site> sites;
	for (uint32_t r = 0; r < n_ref; ++r)
		for (uint64_t x = 0; x < lens[r]; ++x) {
			const uint32_t *c = cnt.data() + 4u * (first[r] + x);
			const uint64_t dp = (uint64_t)c[0] + c[1] + c[2] + c[3];
			if (!dp) continue;
			const char letter = (char)(seqs[r][x] >= 'a' && seqs[r][x] <= 'z' ? seqs[r][x] - 'a' + 'A' : seqs[r][x]);
			const char *at = strchr("ACGT", letter);
			if (!letter || !at) continue;
			const uint32_t ref = (uint32_t)(at - "ACGT");
			bool site = false;
			for (uint32_t b = 0; b < 4u; ++b) site |= b != ref && c[b] >= R.min_alt && (uint64_t)c[b] * 100u >= (uint64_t)R.min_pct * dp;
			if (site) sites.push_back(Site{(first[r] + x) | (uint64_t)ref << REF_SHIFT, {c[0], c[1], c[2], c[3]}});
		}
	out->sites_s = since(t);
	t = Clock::now();
	const int rc = format_sites(sites.data(), sites.size(), n_ref, names, lens, R, command, out);
	out->format_s = since(t);
	return rc;
}

}  // namespace pileup
}  // namespace urx

using namespace urx::pileup;

extern "C" {

void urmapx_pileup_free(urmapx_pileup_result *R) {
	if (!R) return;
	free(R->text);
	R->text = nullptr;
	R->text_bytes = 0;
}

uint64_t urmapx_bam_pileup_resident_bytes(uint64_t total_columns, uint32_t n_ref, int seq_resident) {
	return resident_bytes(total_columns, n_ref, segment_columns(), slice_sites(), seq_resident != 0);
}

uint64_t urmapx_bam_pileup_device_bytes(uint64_t total_columns, uint32_t n_ref, uint64_t n_records) {
	return standalone_bytes(total_columns, n_ref, segment_columns(), slice_sites(), n_records, urx::bamsort::DEFAULT_STAGE);
}

int urmapx_bam_pileup_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint8_t *const *seqs,
                           const uint64_t *starts, size_t n_starts, const urmapx_pileup_opts *opts, const char *command, urmapx_pileup_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t columns = 0;
	Rule R;
	int rc = check_input(n_ref, names, lens, seqs, &columns);
	if (!rc) rc = rule_of(opts, &R);
	if (rc) return rc;
	try {
		std::vector<uint64_t> offs;
		rc = urx::depth::scan_for_depth((const uint8_t *)records, n_bytes, n_ref, starts, n_starts, offs);
		if (!rc) rc = pileup_host((const uint8_t *)records, offs, nullptr, n_ref, names, lens, seqs, R, command, out);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	if (rc) urmapx_pileup_free(out);
	return rc;
}

}  // extern "C"
