// stats_host.cpp -- alignment statistics of BAM records without a device (urmapx_bam_stats_host; the rule is in include/urmapx.h
// "Stats"), the one formatter that writes the text from the tables for both versions, and the host arithmetic the device version
// shares (stats.h).  The counting is written apart from stats.hip on purpose -- one record after the other, one base after the other,
// one thread --, so that the two agreeing says something.
#include "stats.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

#include "depth.h"

namespace urx {
namespace stats {

using bamsort::CORE;
using bamsort::load_u32;

uint32_t test_blocks() {
	const char *e = getenv("URMAPX_TEST_STATS_BLOCKS");
	const long long v = e ? atoll(e) : 0;
	return v >= 1 && v <= 65536 ? (uint32_t)v : 0u;
}

namespace {

// the NM of the aux area [a, e): rule 5
bool find_nm(const uint8_t *a, const uint8_t *e, int64_t &nm) {
	auto width = [](uint8_t t) -> uint32_t {
		switch (t) {
		case 'A': case 'c': case 'C': return 1;
		case 's': case 'S': return 2;
		case 'i': case 'I': case 'f': return 4;
		default: return 0;
		}
	};
	while (e - a >= 3) {
		const bool is_nm = a[0] == 'N' && a[1] == 'M';
		const uint8_t t = a[2];
		a += 3;
		const uint64_t left = (uint64_t)(e - a);
		uint64_t size = width(t);
		if (t == 'Z' || t == 'H') {
			const void *z = memchr(a, 0, (size_t)left);
			if (!z) return false;
			size = (uint64_t)((const uint8_t *)z - a) + 1u;
		} else if (t == 'B') {
			if (left < 5 || a[0] == 'A' || !width(a[0])) return false;
			size = 5u + (uint64_t)load_u32(a + 1) * width(a[0]);
		} else if (!size)
			return false;
		if (size > left) return false;
		if (is_nm && (t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I')) {
			switch (t) {
			case 'c': nm = (int8_t)a[0]; break;
			case 'C': nm = a[0]; break;
			case 's': nm = (int16_t)(a[0] | a[1] << 8); break;
			case 'S': nm = a[0] | a[1] << 8; break;
			case 'i': nm = (int32_t)load_u32(a); break;
			default: nm = load_u32(a); break;
			}
			return true;
		}
		a += size;
	}
	return false;
}

uint32_t base_class(uint32_t code, bool rev) {
	uint32_t c;
	switch (code) {
	case 1: c = 0; break;
	case 2: c = 1; break;
	case 4: c = 2; break;
	case 8: c = 3; break;
	case 15: return 4;
	default: return 5;
	}
	return rev ? 3u - c : c;
}

}  // namespace

void count_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, uint64_t *tab) {
	uint64_t *SN = tab + T_SN;
	const size_t n = offs.size() - 1;
	for (size_t i = 0; i < n; ++i) {
		const uint8_t *r = rec + offs[i];
		const uint64_t len = offs[i + 1] - offs[i];
		uint32_t flag = load_u32(r + 16) >> 16;
		if (action && action[i] == bamsort::MD_SET) flag |= 0x400u;
		if (action && action[i] == bamsort::MD_CLEAR) flag &= ~0x400u;
		++SN[SN_RECORDS];
		if (flag & 0x100u) ++SN[SN_SECONDARY];
		if (flag & 0x800u) ++SN[SN_SUPPLEMENTARY];
		if (flag & 0x900u) continue;

		const uint32_t ref = load_u32(r + 4), l_name = r[12], mapq = r[13], next_ref = load_u32(r + 24);
		uint32_t n_cigar = load_u32(r + 16) & 0xFFFFu;
		uint64_t l_seq = load_u32(r + 20);
		const int32_t tlen = (int32_t)load_u32(r + 32);
		const uint8_t *cig = r + CORE + l_name, *aux = r + len, *const end = r + len;
		if ((uint64_t)CORE + l_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq > len) {
			l_seq = 0;
			n_cigar = 0;
		} else
			aux = cig + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq;
		const uint8_t *seq = cig + 4ull * n_cigar, *qual = seq + (l_seq + 1) / 2;
		const bool paired = flag & 1u, mapped = !(flag & 4u), rev = flag & 0x10u, last = flag & 0x80u, dup = flag & 0x400u, mate_unmapped = flag & 8u;

		++SN[SN_READS];
		if (paired) ++SN[SN_PAIRED];
		++SN[last ? SN_LAST : SN_FIRST];
		++SN[mapped ? SN_MAPPED : SN_UNMAPPED];
		if (paired && mapped && (flag & 2u)) ++SN[SN_PROPER];
		if (paired && mapped && !mate_unmapped) {
			++SN[SN_MAPPED_PAIRED];
			if (next_ref != ref) ++SN[SN_MATE_OTHER];
		}
		if (paired && mapped && mate_unmapped) ++SN[SN_SINGLETONS];
		if (mapped && rev) ++SN[SN_REVERSE];
		if (dup) { ++SN[SN_DUP]; SN[SN_BASES_DUP] += l_seq; }
		if (flag & 0x200u) ++SN[SN_QCFAIL];
		if (mapped && mapq == 0) ++SN[SN_MQ0];
		SN[SN_TOTAL_LEN] += l_seq;
		if (l_seq > SN[SN_MAX_LEN]) SN[SN_MAX_LEN] = l_seq;
		tab[T_RL + 2u * (l_seq < RL_MAX ? l_seq : RL_MAX) + (last ? 1u : 0u)] += 1;
		{
			const uint64_t row = ref == 0xFFFFFFFFu || ref >= n_ref ? n_ref : ref;
			++tab[T_RF + 3u * row + (mapped ? 0u : 1u)];
			if (dup) ++tab[T_RF + 3u * row + 2u];
		}

		if (mapped) {
			SN[SN_BASES_MAPPED] += l_seq;
			++tab[T_MQ + mapq];
			uint64_t aligned = 0;
			for (uint32_t k = 0; k < n_cigar; ++k) {
				const uint32_t w = load_u32(cig + 4u * k), op = w & 15u, L = w >> 4;
				if (op == 0u || op == 7u || op == 8u || op == 1u) aligned += L;
				if (op == 4u) SN[SN_SOFT] += L;
				if (op == 1u) {
					SN[SN_BASES_INS] += L;
					if (L) { ++SN[SN_INS]; ++tab[T_ID + 2u * (L < ID_MAX ? L : ID_MAX)]; }
				}
				if (op == 2u) {
					SN[SN_BASES_DEL] += L;
					if (L) { ++SN[SN_DEL]; ++tab[T_ID + 2u * (L < ID_MAX ? L : ID_MAX) + 1u]; }
				}
			}
			SN[SN_BASES_CIGAR] += aligned;
			int64_t nm = 0;
			if (find_nm(aux, end, nm)) {
				++SN[SN_WITH_NM];
				SN[SN_MISMATCHES] += nm > 0 ? (uint64_t)nm : 0u;
				SN[SN_NM_BASES] += aligned;
			}
			if (paired && !mate_unmapped && next_ref == ref && tlen > 0) {
				const uint32_t size = (uint32_t)tlen < IS_MAX ? (uint32_t)tlen : IS_MAX;
				const bool mate_rev = flag & 0x20u;
				const uint32_t kind = !rev && mate_rev ? 0u : rev && !mate_rev ? 1u : 2u;
				++tab[T_IS + 3u * size + kind];
			}
		}

		if (!l_seq) continue;
		const bool has_qual = qual[0] != 0xFFu;
		if (!has_qual) ++SN[SN_NOQUAL];
		uint64_t gc = 0;
		uint64_t *Q = tab + T_Q + (last ? (uint64_t)QUALS * (CYCLES + 1) : 0u);
		for (uint64_t b = 0; b < l_seq; ++b) {
			const uint32_t code = b & 1u ? seq[b >> 1] & 15u : seq[b >> 1] >> 4;
			const uint64_t cyc = rev ? l_seq - 1u - b : b, row = cyc < CYCLES ? cyc : CYCLES;
			++tab[T_BC + BASES * row + base_class(code, rev)];
			if (code == 2u || code == 4u) ++gc;
			if (has_qual) {
				const uint32_t q = qual[b] < QUALS - 1u ? qual[b] : QUALS - 1u;
				++Q[QUALS * row + q];
				SN[SN_QUAL_SUM] += q;
			}
		}
		if (has_qual) SN[SN_QUAL_BASES] += l_seq;
		++tab[T_GC + 100u * gc / l_seq];
	}
}

namespace {

void put(std::string &t, uint64_t v) { t += std::to_string(v); }
// rule 7
void put_quotient(std::string &t, uint64_t num, uint64_t den, uint32_t d) {
	uint64_t p = 1;
	for (uint32_t k = 0; k < d; ++k) p *= 10u;
	unsigned __int128 v = 0;
	if (den) v = ((unsigned __int128)p * num + den / 2u) / den;
	const uint64_t whole = (uint64_t)(v / p), frac = (uint64_t)(v % p);
	put(t, whole);
	t += '.';
	const std::string f = std::to_string(frac);
	t.append(d - f.size(), '0');
	t += f;
}

}  // namespace

int format_tables(const uint64_t *tab, uint32_t n_ref, const char *const *names, const uint32_t *lens, const char *command, urmapx_stats_result *out) {
	const uint64_t *SN = tab + T_SN;
	std::string t;
	t += "# urmapx stats 1\n# command: ";
	t += command ? command : "";
	t += '\n';
	auto sn = [&](const char *name, uint64_t v) { t += "SN\t"; t += name; t += '\t'; put(t, v); t += '\n'; };
	auto snq = [&](const char *name, uint64_t num, uint64_t den, uint32_t d) { t += "SN\t"; t += name; t += '\t'; put_quotient(t, num, den, d); t += '\n'; };
	// the insert sizes' totals
	uint64_t kinds[3] = {0, 0, 0}, pairs = 0, size_sum = 0, median = 0;
	for (uint32_t s = 0; s <= IS_MAX; ++s)
		for (uint32_t k = 0; k < 3; ++k) {
			const uint64_t c = tab[T_IS + 3u * s + k];
			kinds[k] += c; pairs += c; size_sum += c * s;
		}
	if (pairs) {
		const uint64_t want = (pairs + 1u) / 2u;
		uint64_t seen = 0;
		for (uint32_t s = 0; s <= IS_MAX; ++s) {
			seen += tab[T_IS + 3u * s] + tab[T_IS + 3u * s + 1u] + tab[T_IS + 3u * s + 2u];
			if (seen >= want) { median = s; break; }
		}
	}
	sn("records", SN[SN_RECORDS]);
	sn("secondary", SN[SN_SECONDARY]);
	sn("supplementary", SN[SN_SUPPLEMENTARY]);
	sn("reads", SN[SN_READS]);
	sn("reads paired", SN[SN_PAIRED]);
	sn("first fragments", SN[SN_FIRST]);
	sn("last fragments", SN[SN_LAST]);
	sn("reads mapped", SN[SN_MAPPED]);
	sn("reads unmapped", SN[SN_UNMAPPED]);
	sn("reads properly paired", SN[SN_PROPER]);
	sn("reads mapped and paired", SN[SN_MAPPED_PAIRED]);
	sn("singletons", SN[SN_SINGLETONS]);
	sn("mate on another reference", SN[SN_MATE_OTHER]);
	sn("reads reverse strand", SN[SN_REVERSE]);
	sn("reads duplicated", SN[SN_DUP]);
	sn("reads QC failed", SN[SN_QCFAIL]);
	sn("reads MQ0", SN[SN_MQ0]);
	sn("reads without qualities", SN[SN_NOQUAL]);
	sn("total length", SN[SN_TOTAL_LEN]);
	sn("bases mapped", SN[SN_BASES_MAPPED]);
	sn("bases mapped (cigar)", SN[SN_BASES_CIGAR]);
	sn("bases soft clipped", SN[SN_SOFT]);
	sn("bases inserted", SN[SN_BASES_INS]);
	sn("bases deleted", SN[SN_BASES_DEL]);
	sn("insertions", SN[SN_INS]);
	sn("deletions", SN[SN_DEL]);
	sn("bases duplicated", SN[SN_BASES_DUP]);
	sn("reads with NM", SN[SN_WITH_NM]);
	sn("mismatches", SN[SN_MISMATCHES]);
	snq("error rate", SN[SN_MISMATCHES], SN[SN_NM_BASES], 6);
	snq("average length", SN[SN_TOTAL_LEN], SN[SN_READS], 2);
	sn("maximum length", SN[SN_MAX_LEN]);
	snq("average quality", SN[SN_QUAL_SUM], SN[SN_QUAL_BASES], 2);
	sn("pairs with insert size", pairs);
	sn("inward pairs", kinds[0]);
	sn("outward pairs", kinds[1]);
	sn("other pairs", kinds[2]);
	snq("insert size average", size_sum, pairs, 2);
	sn("insert size median", median);

	for (uint32_t l = 0; l <= RL_MAX; ++l) {
		const uint64_t a = tab[T_RL + 2u * l], b = tab[T_RL + 2u * l + 1u];
		if (a | b) { t += "RL\t"; put(t, l); t += '\t'; put(t, a); t += '\t'; put(t, b); t += '\n'; }
	}
	for (uint32_t q = 0; q < 256u; ++q)
		if (tab[T_MQ + q]) { t += "MQ\t"; put(t, q); t += '\t'; put(t, tab[T_MQ + q]); t += '\n'; }
	for (uint32_t s = 0; s <= IS_MAX; ++s) {
		const uint64_t *c = tab + T_IS + 3u * s;
		if (c[0] | c[1] | c[2]) {
			t += "IS\t"; put(t, s); t += '\t'; put(t, c[0] + c[1] + c[2]);
			for (uint32_t k = 0; k < 3; ++k) { t += '\t'; put(t, c[k]); }
			t += '\n';
		}
	}
	// a table per cycle: rows 1 .. the last one below CYCLES with a count, then the shared row
	auto cycles = [&](const char *tag, const uint64_t *T, uint32_t width) {
		auto any = [&](uint32_t row) {
			for (uint32_t k = 0; k < width; ++k)
				if (T[(uint64_t)width * row + k]) return true;
			return false;
		};
		uint32_t rows = CYCLES;
		while (rows && !any(rows - 1)) --rows;
		for (uint32_t row = 0; row <= CYCLES; ++row) {
			if (row == CYCLES ? !any(row) : row >= rows) continue;
			t += tag; t += '\t';
			if (row == CYCLES) { t += '>'; put(t, CYCLES); } else put(t, row + 1u);
			for (uint32_t k = 0; k < width; ++k) { t += '\t'; put(t, T[(uint64_t)width * row + k]); }
			t += '\n';
		}
	};
	cycles("FFQ", tab + T_Q, QUALS);
	cycles("LFQ", tab + T_Q + (uint64_t)QUALS * (CYCLES + 1), QUALS);
	cycles("BC", tab + T_BC, BASES);
	for (uint32_t g = 0; g <= 100u; ++g)
		if (tab[T_GC + g]) { t += "GC\t"; put(t, g); t += '\t'; put(t, tab[T_GC + g]); t += '\n'; }
	for (uint32_t l = 0; l <= ID_MAX; ++l) {
		const uint64_t a = tab[T_ID + 2u * l], b = tab[T_ID + 2u * l + 1u];
		if (a | b) { t += "ID\t"; put(t, l); t += '\t'; put(t, a); t += '\t'; put(t, b); t += '\n'; }
	}
	for (uint32_t r = 0; r <= n_ref; ++r) {
		const uint64_t *c = tab + T_RF + 3u * (uint64_t)r;
		t += "RF\t";
		if (r < n_ref) { t += names[r]; t += '\t'; put(t, lens[r]); } else t += "*\t0";
		for (uint32_t k = 0; k < 3; ++k) { t += '\t'; put(t, c[k]); }
		t += '\n';
	}

	out->records = SN[SN_RECORDS];
	out->reads = SN[SN_READS];
	out->mapped = SN[SN_MAPPED];
	out->properly_paired = SN[SN_PROPER];
	out->duplicated = SN[SN_DUP];
	out->insert_median = median;
	out->text = (char *)malloc(t.size() ? t.size() : 1);
	if (!out->text) return URMAPX_E_NOMEM;
	memcpy(out->text, t.data(), t.size());
	out->text_bytes = t.size();
	return URMAPX_OK;
}

int stats_host(const uint8_t *rec, const std::vector<uint64_t> &offs, const uint8_t *action, uint32_t n_ref, const char *const *names, const uint32_t *lens,
               const char *command, urmapx_stats_result *out) {
	using Clock = std::chrono::steady_clock;
	auto since = [](Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); };
	auto t = Clock::now();
	std::vector<uint64_t> tab((size_t)table_words(n_ref), 0);
	count_host(rec, offs, action, n_ref, tab.data());
	out->count_s = since(t);
	t = Clock::now();
	const int rc = format_tables(tab.data(), n_ref, names, lens, command, out);
	out->format_s = since(t);
	return rc;
}

}  // namespace stats
}  // namespace urx

using namespace urx::stats;

extern "C" {

void urmapx_stats_free(urmapx_stats_result *R) {
	if (!R) return;
	free(R->text);
	R->text = nullptr;
	R->text_bytes = 0;
}

uint64_t urmapx_bam_stats_resident_bytes(uint32_t n_ref) { return resident_bytes(n_ref); }

int urmapx_bam_stats_host(const void *records, size_t n_bytes, uint32_t n_ref, const char *const *names, const uint32_t *lens, const uint64_t *starts,
                          size_t n_starts, const char *command, urmapx_stats_result *out) {
	if (!out || (n_bytes && !records) || (n_starts && !starts)) return URMAPX_E_ARG;
	memset(out, 0, sizeof *out);
	uint64_t entries = 0;
	int rc = urx::depth::check_refs(n_ref, names, lens, &entries);
	if (rc) return rc;
	try {
		std::vector<uint64_t> offs;
		rc = urx::depth::scan_for_depth((const uint8_t *)records, n_bytes, n_ref, starts, n_starts, offs);
		if (!rc) rc = stats_host((const uint8_t *)records, offs, nullptr, n_ref, names, lens, command, out);
	} catch (const std::bad_alloc &) {
		rc = URMAPX_E_NOMEM;
	}
	if (rc) urmapx_stats_free(out);
	return rc;
}

}  // extern "C"
