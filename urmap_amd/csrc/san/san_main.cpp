// san_main.cpp -- driver of the sanitizer builds (make san): the host side of the drop-in path run from the command line, with the
// device side replaced by san/stub_device.cpp.  tests/test_sanitizers_cpu.py runs it on well-formed and on damaged input; a
// sanitizer report ends the process with exit code 99 (ASAN_OPTIONS / UBSAN_OPTIONS / TSAN_OPTIONS exitcode, set by the tests).
//   urmap_san map <fastq1> [-2 fastq2] -o out.sam [-tab out.tab] [-batch N] [-streams K] [-gpus N] [-shards N] [-threads T] [-null] [-bgzf] [-bam] [-sort] [-markdup] [-sortmem N[G]] [-depth FILE [-depthq N]] [-stats FILE] [-biglen N] [-tags MASK] [-rg LINE]
//       (-tags: URMAPX_TAG_* bits, -rg: an @RG line with real tabs; both need the stand-in store, which exists with -biglen up to 60 000 000)
//       (-biglen: bases of the stand-in index's third sequence, 4 000 000 000 unless given; a BAM position holds 2^31 - 1)
//   urmap_san gunzip <in.gz> <out> [threads]
//   urmap_san fastq <file> <batch>
//   urmap_san makeufi <fasta> <out.ufi> <slots>
//   urmap_san plan <n_bytes> <n_records> <markdup 0|1>     (urmapx_bam_sort_plan_for over a sweep of budgets)
// Exit code: 0 = the call succeeded, 1 = it refused its input with an error code (printed), 2 = usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/urmapx.h"

extern "C" urmapx_index *urx_stub_index(uint32_t n, const uint32_t *lengths, const char *const *labels);

// urmapx_bam_stats_host on a built-in input: a mapped pair with an insertion, a deletion and NM behind a Z field, a reversed read of
// 1 030 bases without qualities, an unmapped read whose SEQ leaves its block, a secondary record, an aux area cut inside a field.
// -> 0 if the call succeeded and counted the records
static int stats_self_check() {
	std::vector<uint8_t> in;
	auto u32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) in.push_back((uint8_t)(v >> (8 * k))); };
	auto record = [&](int32_t ref, int32_t pos, uint32_t flag, uint32_t mapq, const std::vector<uint32_t> &cigar, uint32_t l_seq, uint32_t seq_written, uint8_t qual,
	                  int32_t next_ref, int32_t tlen, const std::string &aux) {
		const size_t at = in.size();
		u32(0);
		u32((uint32_t)ref); u32((uint32_t)pos); u32(2u | mapq << 8 | 4680u << 16); u32((uint32_t)cigar.size() | flag << 16); u32(l_seq);
		u32((uint32_t)next_ref); u32((uint32_t)pos); u32((uint32_t)tlen);
		in.push_back('r'); in.push_back(0);
		for (uint32_t c : cigar) u32(c);
		for (uint32_t k = 0; k < (seq_written + 1) / 2; ++k) in.push_back((uint8_t)(0x12 + 0x11 * (k % 7)));
		for (uint32_t k = 0; k < seq_written; ++k) in.push_back(qual);
		in.insert(in.end(), aux.begin(), aux.end());
		const uint32_t size = (uint32_t)(in.size() - at - 4);
		for (int k = 0; k < 4; ++k) in[at + (size_t)k] = (uint8_t)(size >> (8 * k));
	};
	record(0, 100, 0x63, 40, {50u << 4, 2u << 4 | 1u, 3u << 4 | 2u, 48u << 4}, 100, 100, 30, 0, 300, std::string("XAZab\0NMC\3", 10));
	record(0, 250, 0x93, 40, {100u << 4}, 100, 100, 94, 0, -300, "NMi\1\0\0\0");
	record(1, 7, 0x10, 0, {1030u << 4}, 1030, 1030, 0xFF, -1, 0, "");
	record(-1, -1, 0x4, 0, {}, 5000, 10, 20, -1, 0, "");
	record(0, 5, 0x100, 3, {4u << 4}, 4, 4, 20, -1, 0, "");
	record(2, 9, 0, 9, {4u << 4 | 4u}, 4, 4, 20, -1, 0, "XBBi\2\0\0\0\1");
	static const char *const names[3] = {"chrA", "chrB a label with spaces", "chrBig"};
	const uint32_t lens[3] = {1000000u, 250000u, 0u};
	urmapx_stats_result R;
	const int rc = urmapx_bam_stats_host(in.data(), in.size(), 3, names, lens, nullptr, 0, "urmap_san", &R);
	const bool ok = rc == URMAPX_OK && R.records == 6 && R.reads == 5 && R.mapped == 4 && R.properly_paired == 2 && R.insert_median == 300 && R.text_bytes > 1000;
	if (rc == URMAPX_OK) urmapx_stats_free(&R);
	if (!ok) printf("stats self-check failed: rc=%d\n", rc);
	return ok ? 0 : 1;
}

static int cmd_map(int argc, char **argv) {
	const char *fq1 = argv[0], *fq2 = nullptr, *sam = nullptr, *tab = nullptr;
	urmapx_map_options o;
	memset(&o, 0, sizeof o);
	o.gpus = 1; o.streams = 2; o.minq = 10; o.cmdline = "urmap_san";
	uint32_t biglen = 4000000000u;
	for (int i = 1; i < argc; ++i) {
		const std::string a = argv[i];
		auto val = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
		if (a == "-2") fq2 = val();
		else if (a == "-o") sam = val();
		else if (a == "-tab") tab = val();
		else if (a == "-batch") o.batch = (uint32_t)atoi(val());
		else if (a == "-streams") o.streams = atoi(val());
		else if (a == "-gpus") o.gpus = atoi(val());
		else if (a == "-shards") o.sam_shards = atoi(val());
		else if (a == "-threads") o.host_threads = atoi(val());
		else if (a == "-null") o.discard_sam = 1;
		else if (a == "-bgzf") o.bgzf = 1;
		else if (a == "-bam") o.bam = 1;
		else if (a == "-sort") o.bam_sort = 1;
		else if (a == "-markdup") o.markdup = 1;
		else if (a == "-sortmem") {  // bytes, with G for 2^30
			char *end = nullptr;
			o.sort_mem = strtoull(val(), &end, 10);
			if (end && *end == 'G') o.sort_mem <<= 30;
		}
		else if (a == "-depth") o.depth_out = val();
		else if (a == "-depthq") o.depth_mapq = (uint32_t)atoi(val());
		else if (a == "-stats") o.stats_out = val();
		else if (a == "-tags") o.tags = (unsigned)atoi(val());
		else if (a == "-rg") o.read_group = val();
		else if (a == "-biglen") biglen = (uint32_t)strtoul(val(), nullptr, 10);
		else return 2;
	}
	if (stats_self_check()) return 1;
	const uint32_t lengths[3] = {1000000u, 250000u, biglen};
	static const char *const labels[3] = {"chrA", "chrB a label with spaces", "chrBig"};
	urmapx_index *I = urx_stub_index(3, lengths, labels);
	urmapx_map_report rep;
	char err[512];
	const int rc = urmapx_map_files(I, &o, fq1, fq2, sam, tab, &rep, err, sizeof err);
	if (o.markdup && rc == URMAPX_OK)
		printf("markdup pairs=%llu pair_dups=%llu fragments=%llu fragment_dups=%llu\n", (unsigned long long)rep.pairs_examined, (unsigned long long)rep.pairs_duplicate,
		       (unsigned long long)rep.fragments_examined, (unsigned long long)rep.fragments_duplicate);
	if (o.depth_out && rc == URMAPX_OK)
		printf("depth runs=%llu covered=%llu bases=%llu\n%s", (unsigned long long)rep.depth_runs, (unsigned long long)rep.depth_covered, (unsigned long long)rep.depth_bases,
		       urmapx_map_depth_summary());
	if (o.stats_out && rc == URMAPX_OK)
		printf("stats reads=%llu mapped=%llu properly_paired=%llu duplicated=%llu insert_median=%llu\n", (unsigned long long)rep.stats_reads, (unsigned long long)rep.stats_mapped,
		       (unsigned long long)rep.stats_properly_paired, (unsigned long long)rep.stats_duplicated, (unsigned long long)rep.stats_insert_median);
	printf("rc=%d reads=%llu mapped_q=%llu mapped_lowq=%llu unmapped=%llu text_on_device=%d input_bytes=%llu shards=%d lanes=%d err=%s\n", rc, (unsigned long long)rep.reads,
	       (unsigned long long)rep.mapped_q, (unsigned long long)rep.mapped_lowq, (unsigned long long)rep.unmapped, rep.text_on_device, (unsigned long long)rep.input_bytes, rep.shards,
	       rep.lanes, err);
	urmapx_index_close(I);
	urmapx_host_pool_trim();
	return rc == URMAPX_OK ? 0 : 1;
}

static int cmd_gunzip(int argc, char **argv) {
	if (argc < 2) return 2;
	uint64_t st[3] = {0, 0, 0};
	const int rc = urmapx_gunzip_file(argv[0], argv[1], argc > 2 ? atoi(argv[2]) : 0, st);
	printf("rc=%d bytes=%llu parallel=%llu zlib=%llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]);
	return rc == URMAPX_OK ? 0 : 1;
}

static int cmd_fastq(int argc, char **argv) {
	if (argc < 2) return 2;
	urmapx_fastq *f = nullptr;
	int rc = urmapx_fastq_open(argv[0], &f);
	if (rc) { printf("rc=%d open\n", rc); return 1; }
	const uint32_t batch = (uint32_t)atoi(argv[1]);
	uint64_t n = 0, bases_total = 0, h = 1469598103934665603ull;
	for (;;) {
		const uint8_t *bases, *quals;
		const uint64_t *offs, *loffs;
		const char *ldata;
		const int64_t k = urmapx_fastq_next(f, batch ? batch : 1, &bases, &quals, &offs, &ldata, &loffs);
		if (k < 0) { printf("rc=%lld records=%llu err=%s\n", (long long)k, (unsigned long long)n, urmapx_fastq_error(f)); urmapx_fastq_close(f); return 1; }
		if (k == 0) break;
		for (int64_t i = 0; i < k; ++i) {
			for (uint64_t p = offs[i]; p < offs[i + 1]; ++p) h = ((h ^ bases[p]) * 1099511628211ull ^ quals[p]) * 1099511628211ull;
			for (const char *c = ldata + loffs[i]; *c; ++c) h = (h ^ (unsigned char)*c) * 1099511628211ull;
		}
		n += (uint64_t)k;
		bases_total += offs[k];
	}
	printf("rc=0 records=%llu bases=%llu digest=%016llx\n", (unsigned long long)n, (unsigned long long)bases_total, (unsigned long long)h);
	urmapx_fastq_close(f);
	return 0;
}

static int cmd_makeufi(int argc, char **argv) {
	if (argc < 3) return 2;
	const int rc = urmapx_make_ufi(argv[0], argv[1], 24, 32, strtoull(argv[2], nullptr, 10));
	printf("rc=%d\n", rc);
	return rc == URMAPX_OK ? 0 : 1;
}

// the sort's plan over a sweep of budgets: host arithmetic, so whole-genome sizes cost nothing
static int cmd_plan(int argc, char **argv) {
	if (argc < 3) return 2;
	const uint64_t n_bytes = strtoull(argv[0], nullptr, 10), n_records = strtoull(argv[1], nullptr, 10);
	const int markdup = atoi(argv[2]);
	uint64_t before = ~(uint64_t)0;
	for (uint64_t budget = 1; budget < (uint64_t)1 << 40; budget += budget / 3 + 1) {
		urmapx_bam_sort_plan p;
		const int rc = urmapx_bam_sort_plan_for((size_t)n_bytes, n_records, markdup, budget, &p);
		if (rc == URMAPX_OK && (p.device_bytes > budget || p.partitions > before)) { printf("rc=%d budget=%llu: a plan beyond its budget\n", rc, (unsigned long long)budget); return 1; }
		if (rc == URMAPX_OK) before = p.partitions;
	}
	printf("rc=0 partitions=%llu\n", (unsigned long long)before);
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	const std::string cmd = argv[1];
	if (cmd == "plan") return cmd_plan(argc - 2, argv + 2);
	if (cmd == "map") return cmd_map(argc - 2, argv + 2);
	if (cmd == "gunzip") return cmd_gunzip(argc - 2, argv + 2);
	if (cmd == "fastq") return cmd_fastq(argc - 2, argv + 2);
	if (cmd == "makeufi") return cmd_makeufi(argc - 2, argv + 2);
	return 2;
}
