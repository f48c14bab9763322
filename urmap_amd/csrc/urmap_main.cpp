// urmap_main.cpp -- command line of the MI355X build: the reference's `urmap -map` / `-make_ufi` surface
// (urmap_main.cpp:6-41, map.cpp:27-67, ufindexio.cpp:117-179) as a batch dispatcher over liburmapx.so.
//
//   urmap -map reads.fq[.gz] -ufi index.ufi -samout out.sam [-veryfast] [-threads N] [-gpu D] [-gpus N] [-streams K] [-batch N]
//   urmap -make_ufi genome.fa -output index.ufi [-slots N] [-wordlength W] [-maxix M] [-veryfast] [-gpu D | -host]
//
//   urmap -map2 R1.fq -reverse R2.fq -ufi index.ufi -samout out.sam [-tabbedout out.tab]   (paired-end, map2.cpp:39-90)
//   urmap -ufi_validate index.ufi [-gpu D]                                                   (ufistats.cpp:141-147, on the device)
//   urmap -ufi_stats index.ufi [-log F] [-gpu D] [-quiet]                                    (ufistats.cpp:5-131; ufi_stats.hip)
//   urmap -ufi_counts index.ufi -output F [-gpu D]                                          (ufistats.cpp:133-140, on the device)
//   urmap -ufi_info index.ufi [-log F]                                                      (ufistats.cpp:148-175: the header only)
//
//   urmap -make_bitvec ref.fa -input2 exclude.fa -wordlength W -output x.bv [-gpu D]          (makebitvec.cpp: k-mer bit vector)
//   urmap -search_bitvec reads.fq -ref x.bv -output hits.fq [-trunclabels] [-gpu D]          (searchbitvec.cpp)
//   urmap -search_bitvec2 R1.fq -reverse R2.fq -ref x.bv -output1 h1.fq -output2 h2.fq      (searchbitvec2.cpp; bitvec.hip)
//
// Pipeline of -map: one reader thread parses FASTQ into batches; batch b goes to mapping lane b mod (N*K), a host
// thread with its own mapping context on GPU D + (b mod N) (-gpus N devices, each holding its own replica of the index,
// -streams K contexts per device so that one lane's copies overlap another's kernels); a writer thread takes the
// batches back in input order and formats and writes their SAM.  The reference fans reads over its OpenMP threads the
// same way (map.cpp:58-61, seqsource.cpp:30-66) but writes in completion order; here records are written
// in input order.  No data moves between devices.  Errors: message on stderr, exit status 1
// (myutils.cpp:915), as the reference.
#include <fcntl.h>
#include <omp.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/urmapx.h"
#include "sam.h"

using namespace urx;

[[noreturn]] static void die(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "\n---Fatal error---\n");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	exit(1);
}

struct Opts {
	std::string map, map2, reverse, make_ufi, ufi, ufi_validate, ufi_stats, ufi_counts, ufi_info, samout, tabbedout, output, log;
	std::string make_bitvec, search_bitvec, search_bitvec2, input2, ref, output1, output2;
	bool bgzf = false;  // -bgzf: -samout is a BGZF file, deflated on the device
	std::string bamout; // -bamout: a BAM file in -samout's place, records encoded and deflated on the device
	bool veryfast = false, quiet = false, minq_given = false, host_build = false, notrunclabels = false;
	bool sort = false;  // -sort: the -bamout file in coordinate order, with its .bai index
	bool markdup = false;  // -markdup: with -sort, flag 0x400 on the duplicates
	std::string sortmem;   // -sortmem N[K|M|G]: with -sort, the device memory the sort may take
	bool sortmem_given = false;
	std::string depth;     // -depth FILE: with -sort, a bedGraph file of the per-base depth of the records of the -bamout file
	std::string depth_mapq;  // -depth_mapq N: with -depth, the least MAPQ of a record that counts
	bool depth_given = false, depth_mapq_given = false;
	std::string stats;     // -stats FILE: with -sort, a text file of the alignment statistics of the records of the -bamout file
	bool stats_given = false;
	std::string vcf;       // -vcfout FILE: with -sort, a sites-only VCF file of the columns where the records of the -bamout file differ from the reference
	std::string vcf_mapq, vcf_baseq, vcf_min_alt, vcf_min_pct;  // -vcf_mapq N, -vcf_baseq N, -vcf_min_alt N, -vcf_min_pct N: its thresholds
	bool vcf_given = false, vcf_mapq_given = false, vcf_baseq_given = false, vcf_min_alt_given = false, vcf_min_pct_given = false;
	std::string tags, rg;  // -tags NM,MD,AS and -rg '@RG\tID:..': optional fields of the records, the read group's header line
	bool tags_given = false, rg_given = false;
	bool trunclabels = false, wordlength_given = false;
	double load_factor = 0.6;  // myopts.h: FLT_OPT(load_factor, 0.6, ...)
	unsigned threads = 0, wordlength = 24, maxix = 0, minq = 10;
	unsigned long long slots = 0;
	int gpu = 0, gpus = 1, streams = 2, samshards = 0;
	unsigned batch = 1u << 18;
};

// -sortmem's value: digits, then nothing or one of K M G (either case) for powers of 1024.  0: not such a value (or 0, or beyond 64 bits)
static unsigned long long parse_bytes(const std::string &s) {
	size_t k = 0;
	unsigned long long v = 0;
	for (; k < s.size() && s[k] >= '0' && s[k] <= '9'; ++k) {
		if (v > (~0ull - 9u) / 10u) return 0;
		v = v * 10u + (unsigned)(s[k] - '0');
	}
	if (k == 0 || s.size() > k + 1) return 0;
	if (k < s.size()) {
		const char c = (char)(s[k] | 0x20);
		const int shift = c == 'k' ? 10 : c == 'm' ? 20 : c == 'g' ? 30 : -1;
		if (shift < 0 || v > ~0ull >> shift) return 0;
		v <<= shift;
	}
	return v;
}

static Opts parse(int argc, char **argv) {
	Opts o;
	for (int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		while (a.size() > 1 && a[0] == '-' && a[1] == '-') a.erase(0, 1);
		auto val = [&]() -> const char * {
			if (i + 1 >= argc) die("Missing value for option %s", a.c_str());
			return argv[++i];
		};
		if (a == "-map") o.map = val();
		else if (a == "-map2") o.map2 = val();
		else if (a == "-reverse") o.reverse = val();
		else if (a == "-make_ufi") o.make_ufi = val();
		else if (a == "-ufi") o.ufi = val();
		else if (a == "-ufi_validate") o.ufi_validate = val();
		else if (a == "-ufi_stats") o.ufi_stats = val();
		else if (a == "-ufi_counts") o.ufi_counts = val();
		else if (a == "-ufi_info") o.ufi_info = val();
		else if (a == "-samout") o.samout = val();
		else if (a == "-tabbedout") o.tabbedout = val();
		else if (a == "-output") o.output = val();
		else if (a == "-threads") o.threads = (unsigned)atoi(val());
		else if (a == "-wordlength") { o.wordlength = (unsigned)atoi(val()); o.wordlength_given = true; }
		else if (a == "-maxix") o.maxix = (unsigned)atoi(val());
		else if (a == "-slots") o.slots = strtoull(val(), nullptr, 10);
		else if (a == "-minq") { o.minq = (unsigned)atoi(val()); o.minq_given = true; }
		else if (a == "-gpu") o.gpu = atoi(val());
		else if (a == "-gpus") o.gpus = atoi(val());
		else if (a == "-streams") o.streams = atoi(val());
		else if (a == "-samshards") o.samshards = atoi(val());
		else if (a == "-batch") o.batch = (unsigned)atoi(val());
		else if (a == "-veryfast") o.veryfast = true;
		else if (a == "-bgzf") o.bgzf = true;
		else if (a == "-bamout") o.bamout = val();
		else if (a == "-host") o.host_build = true;
		else if (a == "-sort") o.sort = true;
		else if (a == "-markdup") o.markdup = true;
		else if (a == "-sortmem") { o.sortmem = val(); o.sortmem_given = true; }
		else if (a == "-depth") { o.depth = val(); o.depth_given = true; }
		else if (a == "-stats") { o.stats = val(); o.stats_given = true; }
		else if (a == "-depth_mapq") { o.depth_mapq = val(); o.depth_mapq_given = true; }
		else if (a == "-vcfout") { o.vcf = val(); o.vcf_given = true; }
		else if (a == "-vcf_mapq") { o.vcf_mapq = val(); o.vcf_mapq_given = true; }
		else if (a == "-vcf_baseq") { o.vcf_baseq = val(); o.vcf_baseq_given = true; }
		else if (a == "-vcf_min_alt") { o.vcf_min_alt = val(); o.vcf_min_alt_given = true; }
		else if (a == "-vcf_min_pct") { o.vcf_min_pct = val(); o.vcf_min_pct_given = true; }
		else if (a == "-tags") { o.tags = val(); o.tags_given = true; }
		else if (a == "-rg") { o.rg = val(); o.rg_given = true; }
		else if (a == "-quiet") o.quiet = true;
		else if (a == "-log") o.log = val();
		else if (a == "-load_factor") o.load_factor = atof(val());
		else if (a == "-trunclabels") o.trunclabels = true;  // -map: SetSAM cuts the read label at the first blank whatever this says (setsam.cpp); -make_ufi: the default; -search_bitvec*: cut the labels written
		else if (a == "-make_bitvec") o.make_bitvec = val();
		else if (a == "-search_bitvec") o.search_bitvec = val();
		else if (a == "-search_bitvec2") o.search_bitvec2 = val();
		else if (a == "-input2") o.input2 = val();
		else if (a == "-ref") o.ref = val();
		else if (a == "-output1") o.output1 = val();
		else if (a == "-output2") o.output2 = val();
		else if (a == "-notrunclabels") o.notrunclabels = true;
		else die("Unknown option %s", a.c_str());
	}
	return o;
}

// -log FILE (myutils.cpp: the log file every command opens): program line, command line, start time; whatever the
// command Log()s; finish time.  HitStats writes "@rps=" and the report to it (state1.cpp:593-632).
static FILE *g_log = nullptr;
static std::chrono::steady_clock::time_point g_t0;
static void log_open(const Opts &o, int argc, char **argv) {
	if (o.log.empty()) return;
	g_log = fopen(o.log.c_str(), "w");
	if (!g_log) die("Cannot open log file '%s'", o.log.c_str());
	g_t0 = std::chrono::steady_clock::now();
	fprintf(g_log, "urmap (MI355X build)\n");
	for (int i = 0; i < argc; ++i) fprintf(g_log, "%s ", argv[i]);
	const time_t t = time(nullptr);
	fprintf(g_log, "\nStarted %s", asctime(localtime(&t)));
}
static void log_close() {
	if (!g_log) return;
	const time_t t = time(nullptr);
	const unsigned secs = (unsigned)std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t0).count();
	fprintf(g_log, "\nFinished %s", asctime(localtime(&t)));
	fprintf(g_log, "Elapsed time %02u:%02u\n", secs / 60, secs % 60);
	fclose(g_log);
	g_log = nullptr;
}
// ProgressLog (myutils.cpp): the same text to the terminal and to the log file
static void progress_log(bool quiet, const char *fmt, ...) {
	va_list ap;
	if (!quiet) { va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); }
	if (g_log) { va_start(ap, fmt); vfprintf(g_log, fmt, ap); va_end(ap); }
}

// IntToStr (myutils.cpp:1420-1438): the unit steps
static std::string int_to_str(unsigned long long x) {
	char b[64];
	const double d = (double)x;
	if (x < 10000) snprintf(b, sizeof b, "%u", (unsigned)x);
	else if (d < 1e6) snprintf(b, sizeof b, "%.1fk", d / 1e3);
	else if (d < 100e6) snprintf(b, sizeof b, "%.1fM", d / 1e6);
	else if (d < 1e9) snprintf(b, sizeof b, "%.0fM", d / 1e6);
	else if (d < 10e9) snprintf(b, sizeof b, "%.1fG", d / 1e9);
	else if (d < 100e9) snprintf(b, sizeof b, "%.0fG", d / 1e9);
	else snprintf(b, sizeof b, "%.3g", d);
	return std::string(b);
}

static void check(int rc, const char *what) {
	if (rc != URMAPX_OK && rc != URMAPX_E_UNSUPPORTED) die("%s: %s", what, urmapx_strerror(rc));
}

// -tags LIST: a comma-separated non-empty subset of NM, MD, AS in any order; anything else is refused by the word that is wrong
static unsigned parse_tags(const std::string &list) {
	unsigned mask = 0;
	for (size_t at = 0;;) {
		size_t e = list.find(',', at);
		if (e == std::string::npos) e = list.size();
		const std::string w = list.substr(at, e - at);
		const unsigned bit = w == "NM" ? URMAPX_TAG_NM : w == "MD" ? URMAPX_TAG_MD : w == "AS" ? URMAPX_TAG_AS : 0u;
		if (w.empty()) die("-tags %s: empty element '' (a comma-separated list of NM, MD, AS)", list.c_str());
		if (!bit) die("-tags %s: unknown tag '%s' (a comma-separated list of NM, MD, AS)", list.c_str(), w.c_str());
		if (mask & bit) die("-tags %s: tag '%s' is named twice", list.c_str(), w.c_str());
		mask |= bit;
		if (e == list.size()) break;
		at = e + 1;
	}
	return mask;
}

static int cmd_map(const Opts &o, int argc, char **argv) {
	const bool paired = !o.map2.empty();
	const unsigned minq = paired ? o.minq : 10;  // only cmd_map2 reads -minq (map2.cpp:76); -map keeps State1::m_Minq = 10
	if (paired && o.reverse.empty()) die("-reverse required");
	if (o.ufi.empty()) die("-ufi option required");
	if (o.gpus < 1 || o.gpus > 64) die("-gpus must be 1..64");
	if (o.streams < 1 || o.streams > 8) die("-streams must be 1..8");
	if (o.samshards < 0 || o.samshards > 64) die("-samshards must be 0..64");
	const bool bam = !o.bamout.empty();
	if (bam && !o.samout.empty()) die("-bamout replaces -samout: give one of the two");
	if (bam && o.bgzf) die("-bgzf goes with -samout: a -bamout file is always BGZF");
	const std::string &samout = bam ? o.bamout : o.samout;
	if (o.markdup && !o.sort) die("-markdup needs -sort: the duplicates are marked while the records of the -bamout file are sorted");
	unsigned long long sort_mem = 0;
	if (o.sortmem_given) {
		if (!o.sort) die("-sortmem needs -sort: it is the device memory the sort of the -bamout file may take");
		sort_mem = parse_bytes(o.sortmem);
		if (!sort_mem) die("-sortmem %s: a number of bytes from 1 on, with K, M or G behind it for powers of 1024", o.sortmem.c_str());
	}
	unsigned depth_mapq = 0;
	if (o.depth_mapq_given) {
		if (!o.depth_given) die("-depth_mapq needs -depth: it is the least MAPQ of a record that the depth file counts");
		char *end = nullptr;
		const unsigned long v = strtoul(o.depth_mapq.c_str(), &end, 10);
		if (o.depth_mapq.empty() || *end || o.depth_mapq[0] == '-' || v > 255) die("-depth_mapq %s: a MAPQ from 0 to 255", o.depth_mapq.c_str());
		depth_mapq = (unsigned)v;
	}
	if (o.depth_given) {
		struct stat st;
		if (!o.sort) die("-depth needs -sort: the depth is taken while the records of the -bamout file are sorted");
		if (o.depth.empty()) die("-depth needs a file name");
		if (o.depth == o.bamout || o.depth == o.bamout + ".bai") die("-depth %s: that is the -bamout file or its index; the depth needs a file of its own", o.depth.c_str());
		if (stat(o.depth.c_str(), &st) == 0 && !S_ISREG(st.st_mode)) die("-depth needs a file name, not a pipe or %s: the file is written at the end of the run, in pieces", o.depth.c_str());
	}
	if (o.stats_given) {
		struct stat st;
		if (!o.sort) die("-stats needs -sort: the statistics are counted while the records of the -bamout file are sorted");
		if (o.stats.empty()) die("-stats needs a file name");
		if (o.stats == o.bamout || o.stats == o.bamout + ".bai" || (o.depth_given && o.stats == o.depth))
			die("-stats %s: that is the -bamout file, its index or the -depth file; the statistics need a file of their own", o.stats.c_str());
		if (stat(o.stats.c_str(), &st) == 0 && !S_ISREG(st.st_mode)) die("-stats needs a file name, not a pipe or %s: the file is written at the end of the run", o.stats.c_str());
	}
	// -vcfout and its four numbers (defaults: MAPQ 0, base quality 13, 3 reads, 10 per cent)
	unsigned vcf_num[4] = {0, 13, 3, 10};
	{
		const struct { const char *flag; const std::string &text; bool given; unsigned lo, hi; const char *what; } nums[4] = {
		    {"-vcf_mapq", o.vcf_mapq, o.vcf_mapq_given, 0, 255, "a MAPQ from 0 to 255"},
		    {"-vcf_baseq", o.vcf_baseq, o.vcf_baseq_given, 0, 255, "a base quality from 0 to 255"},
		    {"-vcf_min_alt", o.vcf_min_alt, o.vcf_min_alt_given, 1, 0x7FFFFFFFu, "a number of reads from 1 on"},
		    {"-vcf_min_pct", o.vcf_min_pct, o.vcf_min_pct_given, 0, 100, "a percentage from 0 to 100"}};
		for (int k = 0; k < 4; ++k) {
			if (!nums[k].given) continue;
			if (!o.vcf_given) die("%s needs -vcfout: it is a threshold of the sites that file lists", nums[k].flag);
			char *end = nullptr;
			const unsigned long v = strtoul(nums[k].text.c_str(), &end, 10);
			if (nums[k].text.empty() || *end || nums[k].text[0] == '-' || v < nums[k].lo || v > nums[k].hi) die("%s %s: %s", nums[k].flag, nums[k].text.c_str(), nums[k].what);
			vcf_num[k] = (unsigned)v;
		}
	}
	if (o.vcf_given) {
		struct stat st;
		if (!o.sort) die("-vcfout needs -sort: the bases are piled up while the records of the -bamout file are sorted");
		if (o.vcf.empty()) die("-vcfout needs a file name");
		if (o.vcf == o.bamout || o.vcf == o.bamout + ".bai" || (o.depth_given && o.vcf == o.depth) || (o.stats_given && o.vcf == o.stats))
			die("-vcfout %s: that is the -bamout file, its index, the -depth file or the -stats file; the sites need a file of their own", o.vcf.c_str());
		if (stat(o.vcf.c_str(), &st) == 0 && !S_ISREG(st.st_mode)) die("-vcfout needs a file name, not a pipe or %s: the file is written at the end of the run", o.vcf.c_str());
	}
	if (o.sort) {
		struct stat st;
		if (!bam) die("-sort needs -bamout: it sorts the records of a BAM file");
		if (o.samshards > 1) die("-sort goes with one -bamout file, not with -samshards: a sorted file has one index");
		if (stat(o.bamout.c_str(), &st) == 0 && !S_ISREG(st.st_mode)) die("-sort needs a file name for -bamout, not a pipe or %s: the index %s.bai sits beside it", o.bamout.c_str(), o.bamout.c_str());
		if (o.host_build) setenv("URMAPX_HOST_SORT", "1", 1);  // -host: the sort too runs on the host (urmapx_bam_sort_host)
	}
	// -tags / -rg: refused here, before the index is loaded
	unsigned tag_mask = 0;
	std::vector<char> rg_line(o.rg.size() + 1);
	if (o.tags_given) tag_mask = parse_tags(o.tags);
	if (o.rg_given) {
		char why[512];
		if (urmapx_read_group_id(o.rg.c_str(), rg_line.data(), rg_line.size(), nullptr, 0, why, sizeof why)) die("%s", why);
	}
	if ((o.tags_given || o.rg_given) && samout.empty()) die("-tags and -rg go with -samout or -bamout: they are fields of its records");
	const auto t0 = std::chrono::steady_clock::now();
	urmapx_index *I = nullptr;
	// the file streams to the first device (urmapx_index_open_device); URMAPX_HOST_INDEX=1: through host arrays as before (measurement)
	if (getenv("URMAPX_HOST_INDEX")) check(urmapx_index_open(o.ufi.c_str(), &I), ("Reading index " + o.ufi).c_str());
	else {
		const int rc = urmapx_index_open_device(o.ufi.c_str(), getenv("URMAPX_FORCE_DEVICE") ? atoi(getenv("URMAPX_FORCE_DEVICE")) : o.gpu, &I);
		if (rc == URMAPX_E_NODEVICE || rc == URMAPX_E_NOMEM) die("Uploading index to the GPU: %s", urmapx_strerror(rc));  // (the message of the upload step, as before)
		check(rc, ("Reading index " + o.ufi).c_str());
	}
	if (o.veryfast && urmapx_index_max_ix(I) > 3) fprintf(stderr, "\nWARNING: index not optimal for -veryfast\n");
	const double load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	std::string cl;
	for (int i = 0; i < argc; ++i) { cl += argv[i]; cl.push_back(' '); }  // argv joined with trailing spaces (state1.cpp:749-751)
	urmapx_map_options mo;
	memset(&mo, 0, sizeof mo);
	mo.sam_shards = o.samshards;  // -samout out.sam -samshards N: out.sam.0 .. out.sam.N-1, `cat` of them = the one file
	mo.first_gpu = o.gpu; mo.gpus = o.gpus; mo.streams = o.streams; mo.host_threads = (int)o.threads; mo.batch = o.batch;
	mo.veryfast = o.veryfast ? 1 : 0; mo.minq = o.minq; mo.cmdline = cl.c_str();
	mo.bgzf = o.bgzf ? 1 : 0;
	mo.bam = bam ? 1 : 0;
	mo.bam_sort = o.sort ? 1 : 0;
	mo.tags = tag_mask;
	mo.read_group = o.rg_given ? rg_line.data() : nullptr;
	mo.markdup = o.markdup ? 1 : 0;
	mo.sort_mem = sort_mem;
	mo.depth_out = o.depth_given ? o.depth.c_str() : nullptr;
	mo.depth_mapq = depth_mapq;
	mo.stats_out = o.stats_given ? o.stats.c_str() : nullptr;
	mo.vcf_out = o.vcf_given ? o.vcf.c_str() : nullptr;
	mo.vcf_mapq = vcf_num[0]; mo.vcf_baseq = vcf_num[1]; mo.vcf_min_alt = vcf_num[2]; mo.vcf_min_pct = vcf_num[3];
	urmapx_map_report rep;
	memset(&rep, 0, sizeof rep);
	char err[1024];
	const int rc = urmapx_map_files(I, &mo, paired ? o.map2.c_str() : o.map.c_str(), paired ? o.reverse.c_str() : nullptr,
	                                samout.empty() ? nullptr : samout.c_str(), o.tabbedout.empty() ? nullptr : o.tabbedout.c_str(),
	                                &rep, err, sizeof err);
	if (rc != URMAPX_OK && rc != URMAPX_E_UNSUPPORTED) die("%s", err[0] ? err : urmapx_strerror(rc));
	const unsigned long long n_reads = rep.reads, n_accept = rep.mapped_q, n_reject = rep.mapped_lowq, n_nohit = rep.unmapped;
	const double map_s = rep.seconds;
	if (getenv("URMAPX_VERBOSE"))
		fprintf(stderr, "stage busy seconds: parse %.2f, gpu (copies + kernels, summed over %d lanes) %.2f, format %.2f, write %.2f; %d host threads; text on device: %d\n",
		        rep.parse_s, rep.lanes, rep.gpu_s, rep.format_s, rep.write_s, rep.host_threads, (int)rep.text_on_device);
	if (getenv("URMAPX_VERBOSE") || g_log) {  // where the threads ran (NUMA node of each device's PCI function; @any: not pinned)
		if (getenv("URMAPX_VERBOSE")) fprintf(stderr, "placement: %s\n", rep.placement);
		if (g_log) fprintf(g_log, "placement: %s\n", rep.placement);
	}
	if (g_log) fprintf(g_log, "@rps=%.1f\n", map_s > 0 ? (double)n_reads / map_s : 0.0);  // Log("@rps=..."), state1.cpp:607
	if (!o.quiet || g_log) {  // State1::HitStats (state1.cpp:593-632): same lines, sub-second timers, "GPU n" where it says "n threads"; ProgressLog = terminal + log file
		const bool q = o.quiet;
		auto pct = [&](unsigned long long x) { return n_reads ? 100.0 * (double)x / (double)n_reads : 0.0; };
		auto commas = [](unsigned long long x) {  // IntToStrCommas (myutils.cpp:1400-1418)
			std::string d = std::to_string(x), r;
			for (size_t i = 0; i < d.size(); ++i) {
				if (i && (d.size() - i) % 3 == 0) r += ',';
				r += d[i];
			}
			return r;
		};
		progress_log(q, "\n%16.1f  Seconds to load index\n", load_s);
		if (map_s < 180) progress_log(q, "%16.1f  Seconds in mapper\n", map_s);
		else if (map_s < 2 * 60 * 60) progress_log(q, "%16.1f  Minutes in mapper\n", map_s / 60.0);
		else progress_log(q, "%16.1f  Hours in mapper\n", map_s / 3600.0);
		progress_log(q, "%16s  Reads (%s)\n", commas(n_reads).c_str(), int_to_str(n_reads).c_str());
		if (o.gpus == 1) progress_log(q, "%16.0f  Reads/sec. (GPU %d)\n", map_s > 0 ? (double)n_reads / map_s : 0.0, o.gpu);
		else progress_log(q, "%16.0f  Reads/sec. (%d GPUs)\n", map_s > 0 ? (double)n_reads / map_s : 0.0, o.gpus);
		progress_log(q, "%16s  Mapped Q>=%u (%.1f%%)\n", commas(n_accept).c_str(), minq, pct(n_accept));
		progress_log(q, "%16s  Mapped Q< %u (%.1f%%)\n", commas(n_reject).c_str(), minq, pct(n_reject));
		progress_log(q, "%16s  Unmapped (%.1f%%)\n\n", commas(n_nohit).c_str(), pct(n_nohit));
		if ((o.bgzf && !o.samout.empty()) || bam)
			progress_log(q, bam ? "%16s  Bytes of BAM records, %s written as BGZF (%.3f)\n\n" : "%16s  Bytes of SAM text, %s written as BGZF (%.3f)\n\n", commas(rep.sam_text_bytes).c_str(), commas(rep.sam_file_bytes).c_str(),
			             rep.sam_text_bytes ? (double)rep.sam_file_bytes / (double)rep.sam_text_bytes : 0.0);
		if (o.sort) progress_log(q, "%16.3f  Seconds to sort the records and write %s.bai\n\n", rep.sort_s, samout.c_str());
		if (o.depth_given) {
			progress_log(q, "%16.3f  Seconds for the depth: %llu lines in %s, %llu columns covered, %llu bases on them\n", rep.depth_s, (unsigned long long)rep.depth_runs,
			             o.depth.c_str(), (unsigned long long)rep.depth_covered, (unsigned long long)rep.depth_bases);
			progress_log(q, "%s\n", urmapx_map_depth_summary());
		}
		if (o.stats_given)
			progress_log(q, "%16.3f  Seconds for the statistics in %s: %llu reads, %llu mapped, %llu properly paired, %llu duplicated, median insert size %llu\n\n", rep.stats_s,
			             o.stats.c_str(), (unsigned long long)rep.stats_reads, (unsigned long long)rep.stats_mapped, (unsigned long long)rep.stats_properly_paired,
			             (unsigned long long)rep.stats_duplicated, (unsigned long long)rep.stats_insert_median);
		if (o.vcf_given)
			progress_log(q, "%16.3f  Seconds for the pileup in %s: %llu records counted, %llu sites, %llu alternative alleles\n\n", rep.pileup_s, o.vcf.c_str(),
			             (unsigned long long)rep.pileup_records, (unsigned long long)rep.pileup_sites, (unsigned long long)rep.pileup_alt_alleles);
		if (o.markdup)
			progress_log(q, "%16.3f  Seconds to mark duplicates: %llu of %llu pairs, %llu of %llu fragments\n\n", rep.markdup_s, (unsigned long long)rep.pairs_duplicate,
			             (unsigned long long)rep.pairs_examined, (unsigned long long)rep.fragments_duplicate, (unsigned long long)rep.fragments_examined);
		if (o.minq_given && !paired) progress_log(q, "\nWARNING: Option -minq not used\n\n");
	}
	urmapx_index_close(I);
	const unsigned long long n_unsupported = rep.unsupported;
	if (n_unsupported) die("%llu reads fell outside the device path's domain (length or list overflow); their records are not valid", n_unsupported);
	return 0;
}

// first prime >= n (deterministic Miller-Rabin for 64-bit integers)
static uint64_t mulmod64(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((unsigned __int128)a * b % m); }
static uint64_t powmod64(uint64_t a, uint64_t e, uint64_t m) {
	uint64_t r = 1;
	for (a %= m; e; e >>= 1, a = mulmod64(a, a, m))
		if (e & 1) r = mulmod64(r, a, m);
	return r;
}
static bool is_prime64(uint64_t n) {
	if (n < 2) return false;
	for (uint64_t p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
		if (n % p == 0) return n == p;
	}
	uint64_t d = n - 1;
	int r = 0;
	while ((d & 1) == 0) { d >>= 1; ++r; }
	for (uint64_t a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
		uint64_t x = powmod64(a, d, n);
		if (x == 1 || x == n - 1) continue;
		bool comp = true;
		for (int i = 1; i < r && comp; ++i) {
			x = mulmod64(x, x, n);
			if (x == n - 1) comp = false;
		}
		if (comp) return false;
	}
	return true;
}

// GetPrime (prime.cpp:11-21) walks a ladder of 410 primes and returns the first one >= n.  The ladder is regular:
// rung k is the first prime >= t_k with t_0 = 100 and t_(k+1) = trunc(t_k / 0.95) in double arithmetic (every rung of
// the reference's table follows it; tests/test_abi_cpu.py holds the spot checks), so it is generated, not stored.
// Returns 0 past the last rung, where the reference dies.
static uint64_t get_prime(uint64_t n) {
	uint64_t t = 100;
	for (int k = 0; k < 410; ++k) {
		uint64_t p = t;
		while (!is_prime64(p)) ++p;
		if (p >= n) return p;
		t = (uint64_t)((double)t / 0.95);
	}
	return 0;
}

static int cmd_make_ufi(const Opts &o) {
	if (o.output.empty()) die("-output option required");
	uint64_t slots = o.slots;
	if (slots == 0) {
		// cmd_make_ufi (ufindexio.cpp:138-150): slots = GetPrime(file size / load factor 0.6)
		FILE *f = fopen(o.make_ufi.c_str(), "rb");
		if (!f) die("Cannot open %s", o.make_ufi.c_str());
		fseeko(f, 0, SEEK_END);
		const int64_t size = (int64_t)ftello(f);
		fclose(f);
		if (!(o.load_factor > 0)) die("-load_factor must be positive");
		slots = get_prime((uint64_t)(int64_t)((double)size / o.load_factor));  // int64(GenomeSize/LoadFactor), ufindexio.cpp:146
		if (slots == 0) die("GetPrime(%.3g) overflow", (double)size / o.load_factor);
	}
	unsigned maxix = o.maxix ? o.maxix : (o.veryfast ? 3u : 32u);
	// counting passes, head slots and the overflow list on the GPU, the order-dependent inserts on the host; -host (or no
	// usable device) builds everything on the host.  Same bytes either way.
	const unsigned flags = o.notrunclabels ? URMAPX_UFI_KEEP_LABELS : 0u;
	int rc = o.host_build ? URMAPX_E_NODEVICE : urmapx_make_ufi_opts(o.gpu, o.make_ufi.c_str(), o.output.c_str(), o.wordlength, maxix, slots, flags);
	if (rc == URMAPX_E_NODEVICE || (rc == URMAPX_E_NOMEM && !o.host_build)) {  // the GPU passes need ~17 bytes per slot of HBM
		if (!o.host_build) fprintf(stderr, "make_ufi: %s, building on the host\n", rc == URMAPX_E_NOMEM ? "not enough GPU memory for the counting passes" : "no usable GPU");
		rc = urmapx_make_ufi_opts(-1, o.make_ufi.c_str(), o.output.c_str(), o.wordlength, maxix, slots, flags);
	}
	check(rc, "make_ufi");
	return 0;
}

// cmd_ufi_validate (ufistats.cpp:141-147): FromFile + UFIndex::Validate (ufindex.cpp:611-658), the pass itself on the device
// FromFile for the passes that read the table themselves (-ufi_validate, -ufi_stats, -ufi_counts): the file streams to the device, without
// the derived row layouts; URMAPX_HOST_INDEX=1: through host arrays
static urmapx_index *open_resident(const std::string &path, int gpu) {
	urmapx_index *I = nullptr;
	setenv("URMAPX_NO_CHAIN_ROWS", "1", 0);  // the pass reads the table itself; the derived row layout is not needed for it
	if (getenv("URMAPX_HOST_INDEX")) {
		check(urmapx_index_open(path.c_str(), &I), ("Reading index " + path).c_str());
		check(urmapx_index_upload(I, gpu), "index upload");
	} else {  // the file streams to the device (urmapx_index_open_device)
		const int lrc = urmapx_index_open_device(path.c_str(), gpu, &I);
		if (lrc == URMAPX_E_NODEVICE || lrc == URMAPX_E_NOMEM) check(lrc, "index upload");
		check(lrc, ("Reading index " + path).c_str());
	}
	return I;
}

static int cmd_ufi_validate(const Opts &o) {
	urmapx_index *I = open_resident(o.ufi_validate, o.gpu);
	urmapx_validate_report r;
	const int rc = urmapx_index_validate(I, &r);
	if (rc != URMAPX_OK && rc != URMAPX_E_FORMAT) check(rc, "ufi_validate");
	progress_log(o.quiet, "%llu slots, %llu used, %llu rows, %llu positions re-hashed in %.3f s (GPU %d)\n", (unsigned long long)r.slots,
	             (unsigned long long)r.used, (unsigned long long)r.heads, (unsigned long long)r.positions, r.seconds, o.gpu);
	urmapx_index_close(I);
	if (rc == URMAPX_E_FORMAT) {
		// the reference stops at the first failing slot with "WordToSlot != Slot" (ufindex.cpp:642) or a failed assertion
		const char *what = r.bad_hash ? "WordToSlot != Slot" : r.bad_pos ? "Pos >= SeqDataSize" : r.bad_link ? "broken chain link" :
		                   r.bad_len ? "row longer than MaxIx" : "used slots not all on a chain";
		die("%s: first bad slot 0x%llx (%llu hash, %llu position, %llu link, %llu length failures; %llu slots used, %llu reached)", what,
		    (unsigned long long)r.first_bad_slot, (unsigned long long)r.bad_hash, (unsigned long long)r.bad_pos, (unsigned long long)r.bad_link,
		    (unsigned long long)r.bad_len, (unsigned long long)r.used, (unsigned long long)r.reached);
	}
	return 0;
}

// Int64ToStr (myutils.cpp:1440-1458): IntToStr but for its "%.1fM" step, which ends at 10M instead of 100M
static std::string int64_to_str(unsigned long long x) {
	char b[64];
	const double d = (double)x;
	if (x < 10000) snprintf(b, sizeof b, "%u", (unsigned)x);
	else if (d < 1e6) snprintf(b, sizeof b, "%.1fk", d / 1e3);
	else if (d < 10e6) snprintf(b, sizeof b, "%.1fM", d / 1e6);
	else if (d < 1e9) snprintf(b, sizeof b, "%.0fM", d / 1e6);
	else if (d < 10e9) snprintf(b, sizeof b, "%.1fG", d / 1e9);
	else if (d < 100e9) snprintf(b, sizeof b, "%.0fG", d / 1e9);
	else snprintf(b, sizeof b, "%.3g", d);
	return std::string(b);
}

// MemBytesToStr (myutils.cpp:1220-1235)
static std::string mem_bytes_to_str(double x) {
	char b[64];
	if (x < 1e4) snprintf(b, sizeof b, "%.1fb", x);
	else if (x < 1e6) snprintf(b, sizeof b, "%.1fkb", x / 1e3);
	else if (x < 10e6) snprintf(b, sizeof b, "%.1fMb", x / 1e6);
	else if (x < 1e9) snprintf(b, sizeof b, "%.0fMb", x / 1e6);
	else if (x < 100e9) snprintf(b, sizeof b, "%.1fGb", x / 1e9);
	else snprintf(b, sizeof b, "%.0fGb", x / 1e9);
	return std::string(b);
}

static double get_pct(uint64_t x, uint64_t y) { return y ? 100.0 * (double)x / (double)y : 0.0; }  // GetPct (myutils.h:344-345)

// UFIndex::LogStats's report (ufistats.cpp:62-123), the counters printed as the 64-bit values they are
static std::string stats_report(const urmapx_ufi_stats &r) {
	std::string out;
	char b[256];
	auto put = [&](const char *fmt, auto... a) { snprintf(b, sizeof b, fmt, a...); out += b; };
	unsigned maxi = 0;
	for (unsigned i = 0; i < 256; ++i)
		if (r.count_hist[i]) maxi = i;
	if (maxi > 4) maxi = 4;
	for (unsigned i = 0; i <= maxi; ++i) {
		const unsigned long long ch = r.count_hist[i], th = r.trunc_hist[i];
		put("[%3u]  %10llu", i, ch);
		if (i == 0) put("  %7.7s ", "");
		else put("  %7.2f%%", get_pct(ch, r.total));
		if ((i > 1 && i <= r.max_ix) || th != 0) {
			put("  %10llu  ", th);
			put("  %7.2f%%", get_pct(th, ch));
			if (i == 1 && th > 0) put(" <<< TRUNCATED SINGLES");
			if (th > 0 && i > r.max_ix) put(" <<< GT MaxIx %u", (unsigned)r.max_ix);
		}
		out += "\n";
	}
	out += "\n";
	put("%10llu  Word length\n", (unsigned long long)r.word_length);
	put("%10llu  MaxIx\n", (unsigned long long)r.max_ix);
	put("%10llu  Sequence data (%s)\n", (unsigned long long)r.seqdata_size, int_to_str(r.seqdata_size).c_str());
	put("%10llu  Slots (%s)\n", (unsigned long long)r.slots, int64_to_str(r.slots).c_str());
	const std::pair<const char *, uint64_t> rows[] = {
	    {"Indexed", r.indexed}, {"Indexed2", r.indexed2}, {"NotIndexed", r.not_indexed}, {"Wildcard", r.wildcard}, {"Free", r.free},
	    {"Collision", r.collision}, {"SingleBoth", r.single_both}, {"SinglePlus", r.single_plus}, {"End", r.end}, {"Mine", r.mine},
	    {"Other", r.other}, {"Trunc", r.trunc}, {"Trunc2", r.trunc2}, {"LongMine", r.long_mine}, {"LongOther", r.long_other},
	    {"Total", r.total}};
	for (const auto &x : rows) put("%10llu  %s\n", (unsigned long long)x.second, x.first);
	out += "\n";
	return out;
}

// cmd_ufi_stats (ufistats.cpp:126-131): the report goes to the log (Log), and to stderr unless -quiet
static int cmd_ufi_stats(const Opts &o) {
	urmapx_index *I = open_resident(o.ufi_stats, o.gpu);
	urmapx_ufi_stats r;
	const int rc = urmapx_index_stats(I, &r);
	urmapx_index_close(I);
	if (rc == URMAPX_E_FORMAT)
		die("ufi_stats: damaged row at slot 0x%llx (%llu rows with a position past the sequence store or 256 entries or more)",
		    (unsigned long long)r.first_bad_slot, (unsigned long long)r.bad_rows);
	check(rc, "ufi_stats");
	const std::string rep = stats_report(r);
	if (g_log) fputs(rep.c_str(), g_log);
	if (!o.quiet) {
		fputs(rep.c_str(), stderr);
		fprintf(stderr, "position pass %.3f s, slot pass %.3f s (GPU %d)\n", r.position_seconds, r.slot_seconds, o.gpu);
	}
	return 0;
}

// cmd_ufi_counts (ufistats.cpp:133-140): CountSlots, one byte per slot
static int cmd_ufi_counts(const Opts &o) {
	if (o.output.empty()) die("Missing output file name");
	urmapx_index *I = open_resident(o.ufi_counts, o.gpu);
	const uint64_t n = urmapx_index_slot_count(I);
	std::vector<uint8_t> counts(n);
	const int rc = urmapx_index_slot_counts(I, 0, counts.data(), n);
	urmapx_index_close(I);
	check(rc, "ufi_counts");
	FILE *f = fopen(o.output.c_str(), "wb");
	if (!f) die("Cannot create %s", o.output.c_str());
	if (fwrite(counts.data(), 1, n, f) != n || fclose(f) != 0) die("Write error %s", o.output.c_str());
	return 0;
}

// cmd_ufi_info (ufistats.cpp:148-175): the header, without loading the index
static int cmd_ufi_info(const Opts &o) {
	uint32_t w = 0, m = 0, sd = 0;
	uint64_t sc = 0;
	const int rc = urmapx_ufi_info(o.ufi_info.c_str(), &w, &m, &sd, &sc);
	if (rc == URMAPX_E_IO) die("Cannot read %s", o.ufi_info.c_str());
	if (rc == URMAPX_E_FORMAT) die("%s: not a .ufi file (bad magic)", o.ufi_info.c_str());
	check(rc, "ufi_info");
	progress_log(o.quiet, " Word length  %u\n", w);
	progress_log(o.quiet, "       MaxIx  %u\n", m);
	progress_log(o.quiet, "     SeqData  %u (%s)\n", sd, mem_bytes_to_str((double)sd).c_str());
	progress_log(o.quiet, "       Slots  %llu (%s)\n", (unsigned long long)sc, mem_bytes_to_str((double)sc).c_str());
	return 0;
}

// ---- k-mer bit vector (bitvec.hip).  -threads is accepted and has no effect: records are written in input order ----
static void check_bitvec_w(unsigned W) {
	if (W < URMAPX_BV_MIN_W || W > URMAPX_BV_MAX_W)
		die("-wordlength %u: %s (the bit vector takes word lengths %d..%d; 4^W bits)", W, urmapx_strerror(URMAPX_E_UNSUPPORTED), URMAPX_BV_MIN_W,
		    URMAPX_BV_MAX_W);
}

// cmd_make_bitvec (makebitvec.cpp:72-106)
static int cmd_make_bitvec(const Opts &o) {
	if (o.input2.empty()) die("Missing input file name");
	if (o.output.empty()) die("Missing output file name");
	if (!o.wordlength_given) die("-wordlength option required");
	check_bitvec_w(o.wordlength);
	uint64_t counts[2] = {0, 0};
	const int rc = urmapx_make_bitvec(o.gpu, o.make_bitvec.c_str(), o.input2.c_str(), o.wordlength, o.output.c_str(), counts);
	if (rc == URMAPX_E_IO) die("Cannot read %s or write %s", (o.make_bitvec + " / " + o.input2).c_str(), o.output.c_str());
	check(rc, "make_bitvec");
	// the reference passes 64-bit counts to %u (their low 32 bits) and to IntToStr
	progress_log(o.quiet, "%u words included (%s)\n", (unsigned)counts[0], int_to_str(counts[0]).c_str());
	progress_log(o.quiet, "%u words excluded (%s)\n", (unsigned)counts[1], int_to_str(counts[1]).c_str());
	return 0;
}

// cmd_search_bitvec / cmd_search_bitvec2 (searchbitvec.cpp:88-150, searchbitvec2.cpp:64-126)
static int cmd_search_bitvec(const Opts &o) {
	const bool paired = !o.search_bitvec2.empty();
	if (paired && o.reverse.empty()) die("-reverse required");
	if (o.ref.empty()) die("-ref option required");
	if (paired ? (o.output1.empty() || o.output2.empty()) : o.output.empty()) die("Missing output file name");
	{  // the header is checked before a device is opened
		FILE *f = fopen(o.ref.c_str(), "rb");
		if (!f) die("Cannot open %s", o.ref.c_str());
		uint32_t hdr[2] = {0, 0};
		const size_t got = fread(hdr, 4, 2, f);
		fclose(f);
		if (got < 1 || hdr[0] != URMAPX_BV_MAGIC) die("Invalid .bv file");
		if (got < 2) die("Invalid .bv file");
		check_bitvec_w(hdr[1]);
	}
	urmapx_bitvec *B = nullptr;
	const int orc = urmapx_bitvec_open(o.ref.c_str(), o.gpu, &B);
	if (orc == URMAPX_E_FORMAT) die("Invalid .bv file (shorter than its word length says)");
	check(orc, ("Reading bitvec " + o.ref).c_str());
	uint64_t counts[2] = {0, 0};
	char err[1024];
	const int rc = urmapx_search_bitvec_files(B, paired ? o.search_bitvec2.c_str() : o.search_bitvec.c_str(), paired ? o.reverse.c_str() : nullptr,
	                                          paired ? o.output1.c_str() : o.output.c_str(), paired ? o.output2.c_str() : nullptr,
	                                          o.trunclabels ? URMAPX_BV_TRUNC_LABELS : 0u, counts, err, sizeof err);
	urmapx_bitvec_close(B);
	if (rc != URMAPX_OK) die("%s", err[0] ? err : urmapx_strerror(rc));
	progress_log(o.quiet, "%u / %u found (%.1f%%)\n", (unsigned)counts[0], (unsigned)counts[1],
	             counts[1] ? 100.0 * (double)counts[0] / (double)counts[1] : 0.0);
	return 0;
}

int main(int argc, char **argv) {
	setenv("OMP_WAIT_POLICY", "passive", 0);  // idle pool threads sleep: three pipeline stages share the cores
	// The HIP runtime spreads a process's streams over FOUR hardware queues unless told otherwise, and streams that share one take turns: two lanes are four
	// streams (a lane's own and its copy-back stream), beside the loader's.  Before the runtime starts (round 6: the lanes of a process with a few more streams
	// ran at 29 M reads/s instead of 39 M until this was set; profiles/r6/hw_queues.txt).  The library sets the same when it is loaded (urmapx.hip).
	setenv("GPU_MAX_HW_QUEUES", "16", 0);
	Opts o = parse(argc, argv);
	log_open(o, argc, argv);
	if (!o.map.empty() || !o.map2.empty()) { const int rc = cmd_map(o, argc, argv); log_close(); return rc; }
	if (!o.make_ufi.empty()) { const int rc = cmd_make_ufi(o); log_close(); return rc; }
	if (!o.ufi_validate.empty()) { const int rc = cmd_ufi_validate(o); log_close(); return rc; }
	if (!o.ufi_stats.empty()) { const int rc = cmd_ufi_stats(o); log_close(); return rc; }
	if (!o.ufi_counts.empty()) { const int rc = cmd_ufi_counts(o); log_close(); return rc; }
	if (!o.ufi_info.empty()) { const int rc = cmd_ufi_info(o); log_close(); return rc; }
	if (!o.make_bitvec.empty()) { const int rc = cmd_make_bitvec(o); log_close(); return rc; }
	if (!o.search_bitvec.empty() || !o.search_bitvec2.empty()) { const int rc = cmd_search_bitvec(o); log_close(); return rc; }
	fprintf(stderr, "urmap (MI355X build)\n  urmap -map reads.fq -ufi index.ufi -samout out.sam [-veryfast] [-gpu D] [-gpus N] [-streams K] [-samshards N] [-bgzf]\n"
	                "  urmap -map2 R1.fq -reverse R2.fq -ufi index.ufi -samout out.sam [-tabbedout out.tab] [-gpu D] [-gpus N] [-bgzf]\n"
	                "      -bgzf: the file named by -samout is BGZF (gzip members of 64 KB of text, deflated on the GPU); `gzip -dc` gives the SAM text\n"
	                "      -bamout out.bam: in place of -samout, a BAM file (records encoded and deflated on the GPU, unsorted);\n"
	                "               with -samshards N every out.bam.0 .. out.bam.N-1 is a complete BAM file\n"
	                "      -sort: with -bamout, the records in coordinate order (sorted on the GPU) and the index out.bam.bai beside the file\n"
                "      -markdup: with -sort, flag 0x400 on duplicate reads (Picard's rule: same ends, the best qualities stay), marked on the GPU\n"
                "      -depth FILE: with -sort, the per-base depth of the records as written (with -markdup: without the duplicates) as a\n"
                "          bedGraph file, runs of depth 0 included, computed on the GPU beside the sort; a table per reference goes to the log\n"
                "      -depth_mapq N: with -depth, records with a MAPQ below N do not count (0..255; default 0)\n"
                "      -stats FILE: with -sort, the alignment statistics of the records as written -- counts by flag, MAPQ, read lengths, insert\n"
                "          sizes, qualities and bases per cycle, GC, indels, reads per reference -- as a text file, counted on the GPU beside the sort\n"
                "      -vcfout FILE: with -sort, the columns where the records as written show a base other than the reference's, as a sites-only\n"
                "          VCF 4.2 file with DP and AD (SNV candidates; no indels, no genotypes), piled up on the GPU beside the sort\n"
                "      -vcf_mapq N, -vcf_baseq N: with -vcfout, the least MAPQ of a record and the least quality of a base that count (0..255; defaults 0, 13)\n"
                "      -vcf_min_alt N, -vcf_min_pct N: with -vcfout, an alternative allele needs N bases (from 1; default 3) and N per cent of the column's (0..100; default 10)\n"
                "      -sortmem N[K|M|G]: with -sort, the GPU memory the sort may take; records that do not fit it stream through the GPU in partitions\n"
	                "      -tags NM,MD,AS: these optional fields behind QUAL of every mapped record (any subset; computed on the GPU), SAM and BAM\n"
	                "      -rg '@RG\\tID:x\\tSM:y': that line in the header in front of @PG and RG:Z:x on every record\n"
	                "  urmap -make_ufi genome.fa -output index.ufi [-slots N] [-wordlength W] [-maxix M]\n"
	                "  urmap -ufi_validate index.ufi [-gpu D]\n"
	                "  urmap -ufi_stats index.ufi [-log F] [-gpu D] [-quiet]\n"
	                "  urmap -ufi_counts index.ufi -output F [-gpu D]\n"
	                "  urmap -ufi_info index.ufi [-log F]\n"
	                "  urmap -make_bitvec ref.fa -input2 exclude.fa -wordlength W -output x.bv [-gpu D]\n"
	                "  urmap -search_bitvec reads.fq -ref x.bv -output hits.fq [-trunclabels] [-gpu D]\n"
	                "  urmap -search_bitvec2 R1.fq -reverse R2.fq -ref x.bv -output1 h1.fq -output2 h2.fq [-trunclabels] [-gpu D]\n");
	return 0;
}
