// pipeline.cpp -- FASTQ file(s) -> SAM file through the mapping path: cmd_map / cmd_map2 (map.cpp:27-67, map2.cpp:39-90)
// as a library call (urmapx_map_files), so that the command line and an embedding program with an index already resident
// in HBM run the same code.
//
// One reader thread parses FASTQ into batches; batch b goes to mapping lane b mod (N*K), a host thread with its own
// mapping context on GPU first_gpu + (b mod N) (N devices, each holding its own replica of the index; K contexts per
// device so that one lane's copies overlap another's kernels); a writer thread takes the batches back in input order and
// formats and writes their SAM with all host threads.  The reference fans reads over its OpenMP threads the same way
// (map.cpp:58-61, seqsource.cpp:30-66) but writes in completion order; here records are written in input
// order.  No data moves between devices.  The batch arrays that cross PCIe are page-locked once they have their size.
//
// Input from files, .gz files and pipes takes the shorter road first (text phase): the reader cuts the input into chunks at
// record starts and reads them into page-locked buffers, a lane hands the chunk's BYTES to the device and gets the bytes
// of its SAM records back (text_gpu.hip: line ends, record checks, search, SAM text all on the GPU), and the writer
// copies them into the output file.  The host then only moves bytes.  A chunk the device parser does not take as it is
// ends the text phase; the host reader continues at that chunk's first byte with the line count kept, so '\r', blank
// lines and malformed records get the reference's handling and messages.
//
// map_files_impl is open -> text phase -> host phase (if the text phase left work) -> finish.  Run holds what the stages share and
// lets go of it in close(); TextPhase (stream or plain-file reader, lanes, writer) and HostPhase (reader, mate reader, lanes, formatter,
// flusher) hold their channels; each member a thread writes while the others run names that thread.
#include <fcntl.h>
#include <sched.h>
#include <functional>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/vfs.h>
#include <hip/hip_runtime_api.h>
#include <omp.h>
#include <unistd.h>
#include <zlib.h>

#include "pgzip.h"

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/urmapx.h"
#include "internal.h"
#include "sam.h"

using namespace urx;

namespace {

// Page-locks the storage of a PodVec for as long as it keeps its address (hipHostRegister); the vector tells the pin
// before it reallocates or frees, and the next use registers the new storage.
template <class T>
struct Pin {
	PodVec<T> *v = nullptr;
	void *p = nullptr;
	size_t n = 0;
	static void on_free(void *ctx, void *) { static_cast<Pin *>(ctx)->drop(); }
	void hold(PodVec<T> &vec) {
		if (!v) { v = &vec; vec.set_pre_free(&Pin::on_free, this); }
		void *q = vec.data();
		const size_t bytes = vec.capacity() * sizeof(T);
		if (q == p && bytes == n) return;
		drop();
		if (q && bytes && hipHostRegister(q, bytes, hipHostRegisterDefault) == hipSuccess) { p = q; n = bytes; }
		else (void)hipGetLastError();
	}
	void drop() {
		if (p) (void)hipHostUnregister(p);
		p = nullptr; n = 0;
	}
	~Pin() {
		drop();
		if (v) v->set_pre_free(nullptr, nullptr);
	}
};

struct Job {
	FastqBatch reads;
	PodVec<urmapx_result> results;
	PodVec<urmapx_path_op> ops;
	std::vector<urmapx_pair_info> info;  // -tabbedout
	Pin<uint8_t> pin_bases;
	Pin<uint64_t> pin_offs;
	Pin<urmapx_result> pin_results;
	Pin<urmapx_path_op> pin_ops;
};

using Clock = std::chrono::steady_clock;
inline Clock::time_point now() { return Clock::now(); }
inline double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
// thread t's share of n units split over a team of T: [part(n, t, T), part(n, t + 1, T))
inline size_t part(size_t n, int t, int T) { return (size_t)((uint64_t)n * (uint64_t)t / (uint64_t)T); }

// n bytes of fd at `off` into dst; false: an error, or the file ends first
inline bool pread_all(int fd, char *dst, size_t n, uint64_t off) {
	for (size_t got = 0; got < n;) {
		const ssize_t k = pread(fd, dst + got, n - got, (off_t)(off + got));
		if (k <= 0) return false;
		got += (size_t)k;
	}
	return true;
}
// [off, off + n) of a file into dst, by several threads
inline bool read_range(int fd, char *dst, uint64_t off, size_t n, int threads) {
	std::atomic<bool> ok{true};
#pragma omp parallel for schedule(static, 1) num_threads(threads)
	for (int t = 0; t < threads; ++t) {
		const size_t lo = part(n, t, threads), hi = part(n, t + 1, threads);
		if (!pread_all(fd, dst + lo, hi - lo, off + lo)) ok.store(false);
	}
	return ok.load();
}
// number of '\n' in [c, e)
inline size_t count_nl(const char *c, const char *e) {
	size_t n = 0;
	for (const char *nl; c < e && (nl = (const char *)memchr(c, '\n', (size_t)(e - c))); c = nl + 1) ++n;
	return n;
}

template <class T>
class Channel {  // bounded queue
public:
	explicit Channel(size_t cap) : cap_(cap) {}
	void push(T v) {
		std::unique_lock<std::mutex> l(m_);
		cv_.wait(l, [&] { return q_.size() < cap_; });
		q_.push_back(std::move(v));
		cv_.notify_all();
	}
	bool pop(T &v) {
		std::unique_lock<std::mutex> l(m_);
		cv_.wait(l, [&] { return !q_.empty() || closed_; });
		return take(v);
	}
	bool try_pop(T &v) {
		std::lock_guard<std::mutex> l(m_);
		return take(v);
	}
	void close() {
		std::lock_guard<std::mutex> l(m_);
		closed_ = true;
		cv_.notify_all();
	}

private:
	bool take(T &v) {  // under m_
		if (q_.empty()) return false;
		v = std::move(q_.front());
		q_.pop_front();
		cv_.notify_all();
		return true;
	}
	std::mutex m_;
	std::condition_variable cv_;
	std::deque<T> q_;
	size_t cap_;
	bool closed_ = false;
};

// URMAPX_PIPE_TRACE=1: every stage of every chunk with its start and end (ms since the first read), to stderr at the end
struct Trace {
	bool on = getenv("URMAPX_PIPE_TRACE") != nullptr;
	std::mutex m;
	Clock::time_point t0 = now();
	struct Ev { const char *what; int lane; size_t job; double a, b; };
	std::vector<Ev> evs;
	void add(const char *what, int lane, size_t job, Clock::time_point since) {
		if (!on) return;
		std::lock_guard<std::mutex> l(m);
		evs.push_back(Ev{what, lane, job, 1e3 * secs(t0, since), 1e3 * secs(t0, now())});
	}
	void dump() {
		if (!on) return;
		std::sort(evs.begin(), evs.end(), [](const Ev &x, const Ev &y) { return x.a < y.a; });
		for (const Ev &e : evs) fprintf(stderr, "trace %-10s lane %d job %3zu  %9.2f .. %9.2f  (%7.2f ms)\n", e.what, e.lane, e.job, e.a, e.b, e.b - e.a);
	}
};

struct Failure {
	std::atomic<bool> set{false};
	std::mutex m;
	int code = 0;
	std::string msg;
	void raise(int c, const std::string &s) {
		std::lock_guard<std::mutex> l(m);
		if (!set.load()) { code = c; msg = s; set.store(true); }
	}
};


// The SAM file.  Pieces are copied to their offsets by several threads: through a shared mapping of the file where that
// works (parallel page faults; write() on one file is serialised by the inode lock), else with pwrite.
class FileSink {
public:
	~FileSink() { if (fd_ >= 0) ::close(fd_); free(mem_); }
	// bam_sort: the pieces are kept at their offsets in host memory instead (the file is written once they are sorted); write_through()
	// ends that, and what write_at gets from then on goes to the file
	void keep_in_memory() { memory_ = true; }
	void write_through() { memory_ = false; }
	const char *kept() const { return mem_; }
	// where the pieces began, ascending: record starts all of them (urmapx_bam_sort walks the chain from each)
	std::vector<uint64_t> kept_starts() { std::sort(mem_starts_.begin(), mem_starts_.end()); return mem_starts_; }
	void drop_kept() { free(mem_); mem_ = nullptr; mem_cap_ = 0; }
	// measurement (urmapx_map_options.discard_sam): the text is taken and dropped
	void open_discard() { discard_ = true; }
	bool open(const char *path) {
		const char *mode = getenv("URMAPX_SAM_WRITE");  // "pwrite" (default) | "mmap"
		const bool want_map = mode && !strcmp(mode, "mmap");
		fd_ = ::open(path, (want_map ? O_RDWR : O_WRONLY) | O_CREAT | O_TRUNC, 0644);
		if (fd_ < 0 && want_map) fd_ = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (fd_ < 0) return false;
		struct stat st;
		const bool regular = fstat(fd_, &st) == 0 && S_ISREG(st.st_mode);
		sequential_ = !regular;  // a pipe, a FIFO, a terminal (-samout /dev/stdout | ...): bytes go out in order with write()
		use_map_ = regular && want_map;
		return true;
	}
	bool is_open() const { return fd_ >= 0; }
	bool seekable() const { return !sequential_; }
	// Threads that should share one piece's pwrite: on tmpfs (and ramfs) write() is a memcpy under the inode lock -- one
	// thread does 5.8 GB/s, eight together 3.7 (scripts/fs_bench.cpp) -- so one; on a disk file system concurrent pwrites
	// of disjoint ranges overlap their I/O, so a few.
	int writer_threads(int host_threads) const {
		if (discard_) return 1;
		if (const char *e = getenv("URMAPX_WRITE_THREADS")) return std::max(1, atoi(e));
		if (sequential_ || fd_ < 0) return 1;
		return in_memory() != 0 ? 1 : std::max(1, std::min(4, host_threads));
	}
	const char *medium() const {
		if (discard_) return "discarded";
		if (sequential_) return "pipe";
		const int m = fd_ < 0 ? -1 : in_memory();
		return m < 0 ? "file" : m ? "tmpfs" : "disk file system";
	}
	// 1: the file lives on tmpfs or ramfs, 0: on another file system, -1: not known
	int in_memory() const {
		struct statfs fs;
		if (fstatfs(fd_, &fs) != 0) return -1;
		return fs.f_type == 0x01021994L /* tmpfs */ || (long)fs.f_type == (long)0x858458f6L /* ramfs */;
	}
	// makes the file at least `end` bytes long (pieces below `end` can then be written from several threads at once)
	bool reserve(uint64_t end) {
		if (memory_ || !use_map_ || end <= size_) return true;
		if (ftruncate(fd_, (off_t)end) != 0) { use_map_ = false; return true; }
		size_ = end;
		return true;
	}
	bool write_at(const char *p, size_t n, uint64_t off, int threads) {
		if (n == 0 || discard_) return true;
		if (memory_) {  // (pieces arrive from several threads, each at an offset of its own; only growing moves the array)
			std::lock_guard<std::mutex> g(mem_lock_);
			if (off + n > mem_cap_) {
				const size_t want = std::max<size_t>((size_t)(off + n), mem_cap_ + mem_cap_ / 2 + (1u << 20));
				char *m = (char *)realloc(mem_, want);
				if (!m) return false;
				mem_ = m; mem_cap_ = want;
			}
			memcpy(mem_ + off, p, n);
			mem_starts_.push_back(off);
			return true;
		}
		if (threads < 1) threads = 1;
		if (sequential_) {  // the callers hand pieces over in file order when seekable() is false
			if (off != size_) return false;
			size_t done = 0;
			while (done < n) {
				ssize_t w = ::write(fd_, p + done, n - done);
				if (w <= 0) return false;
				done += (size_t)w;
			}
			size_ = off + n;
			return true;
		}
		if (use_map_) {
			if (off + n > size_ && ftruncate(fd_, (off_t)(off + n)) != 0) use_map_ = false;
			else {
				if (off + n > size_) size_ = off + n;
				const uint64_t a = off & ~(uint64_t)4095;
				const size_t len = (size_t)(off + n - a);
				char *m = (char *)mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_SHARED, fd_, (off_t)a);
				if (m == MAP_FAILED) use_map_ = false;
				else {
					char *dst = m + (off - a);
#pragma omp parallel for schedule(static, 1) num_threads(threads)
					for (int t = 0; t < threads; ++t) {
						const size_t lo = part(n, t, threads), hi = part(n, t + 1, threads);
						memcpy(dst + lo, p + lo, hi - lo);
					}
					munmap(m, len);
					return true;
				}
			}
		}
		std::atomic<bool> ok{true};
#pragma omp parallel for schedule(static, 1) num_threads(threads)
		for (int t = 0; t < threads; ++t) {
			const size_t lo = part(n, t, threads), hi = part(n, t + 1, threads);
			size_t done = lo;
			while (done < hi) {
				ssize_t w = pwrite(fd_, p + done, hi - done, (off_t)(off + done));
				if (w <= 0) { ok.store(false); break; }
				done += (size_t)w;
			}
		}
		if (off + n > size_) size_ = off + n;
		return ok;
	}
	bool finish(uint64_t length) {
		if (fd_ < 0 || discard_) return true;
		bool ok = sequential_ || size_ == length || ftruncate(fd_, (off_t)length) == 0;
		ok = ::close(fd_) == 0 && ok;
		fd_ = -1;
		return ok;
	}

private:
	int fd_ = -1;
	bool sequential_ = false, discard_ = false, memory_ = false;
	std::mutex mem_lock_;
	char *mem_ = nullptr;
	size_t mem_cap_ = 0;
	std::vector<uint64_t> mem_starts_;
	std::atomic<bool> use_map_{false};
	std::atomic<uint64_t> size_{0};
};

// -bgzf: text replaced by its BGZF members (urmapx_bgzf_compress_host), for what the host formats: the header, the chunks the device
// parser hands back, the whole -host road
// -bamout: a QNAME that l_read_name cannot hold ends the run (nothing is truncated)
std::string bam_long_name(const char *label) {
	return std::string("QNAME longer than 254 bytes does not fit a BAM record, read ") + label;
}

bool bgzf_members(std::string &text, int with_eof = 0) {
	std::string z;
	z.resize(urmapx_bgzf_bound(text.size()));
	size_t used = 0;
	if (urmapx_bgzf_compress_host(text.data(), text.size(), &z[0], z.size(), &used, with_eof) != URMAPX_OK) return false;
	z.resize(used);
	text.swap(z);
	return true;
}

// Page-locked host buffers are kept for the next call of this process (pinning and unpinning a few hundred MB costs tens
// of milliseconds each way, as much as mapping the chunk that travels in them); urmapx_host_pool_trim() lets go of them.
class HostPool {
public:
	static HostPool &get() { static HostPool *p = new HostPool; return *p; }  // never destroyed: the runtime may be gone by then
	char *acquire(size_t want, size_t &cap) {
		{
			std::lock_guard<std::mutex> l(m_);
			size_t best = free_.size();
			for (size_t i = 0; i < free_.size(); ++i)
				if (free_[i].cap >= want && (best == free_.size() || free_[i].cap < free_[best].cap)) best = i;
			if (best < free_.size() && free_[best].cap <= want + want / 2 + (8u << 20)) {
				char *p = free_[best].p;
				cap = free_[best].cap;
				held_ -= cap;
				free_.erase(free_.begin() + (long)best);
				return p;
			}
		}
		char *p = nullptr;
		if (const char *e = getenv("URMAPX_TEST_PINNED_ALLOCS")) {  // tests: the (N+1)-th fresh allocation of the process fails
			if (fresh_.fetch_add(1) >= (uint64_t)atoll(e)) return nullptr;
		}
		AllocTimer at(1);
		if (hipHostMalloc((void **)&p, want, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		cap = want;
		return p;
	}
	void release(char *p, size_t cap) {
		if (!p) return;
		{
			std::lock_guard<std::mutex> l(m_);
			if (held_ + cap <= kKeep) { free_.push_back(Buf{p, cap}); held_ += cap; return; }
		}
		AllocTimer at(1);
		(void)hipHostFree(p);
	}
	void trim() {
		std::vector<Buf> v;
		{
			std::lock_guard<std::mutex> l(m_);
			v.swap(free_);
			held_ = 0;
		}
		for (const Buf &b : v) (void)hipHostFree(b.p);
	}

private:
	struct Buf { char *p; size_t cap; };
	static constexpr size_t kKeep = (size_t)16 << 30;  // 2 pipelines x 8 chunks of 524 288 reads in flight = 6.3 GB, and the other shapes a process maps (smaller files, mate pairs) beside them
	std::mutex m_;
	std::vector<Buf> free_;
	size_t held_ = 0;
	std::atomic<uint64_t> fresh_{0};
};

// A lane's mapping context and text stage are kept for the next urmapx_map_files call on the same index and device: their
// device arrays (2.5-3 GB per lane: DpJobs, parked states, path arena, the chunk's text both ways) are otherwise allocated in
// the first chunk of every call and freed at its end, and on a device that has just freed as much, hipMalloc has been measured
// at 27 ms a call instead of 0.2 (48 of them per lane: 0.6 s in front of a 0.3 s run; profiles/r5/e2e_watch.txt).
// urmapx_index_close destroys the lanes of its index, urmapx_host_pool_trim all of them; URMAPX_NO_LANE_POOL=1 keeps none.
struct PooledLane {
	const urmapx_index *I;
	int device;
	urmapx_params P;
	bool veryfast, pair_info;
	urmapx_ctx *C;
	urmapx_text *T;
	uint64_t env = 0;  // what the URMAPX_* knobs were when the context was made (a context caches what they decide): reused only under the same
};
// every URMAPX_* variable of the environment, names and values, as one number
uint64_t env_knobs() {
	uint64_t h = 1469598103934665603ull;
	for (char **e = environ; e && *e; ++e)
		if (!strncmp(*e, "URMAPX_", 7) && strncmp(*e, "URMAPX_VERBOSE", 14) && strncmp(*e, "URMAPX_PIPE_TRACE", 17))
			for (const char *c = *e; *c; ++c) h = (h ^ (unsigned char)*c) * 1099511628211ull;
	return h;
}
class LanePool {
public:
	static LanePool &get() { static LanePool *p = new LanePool; return *p; }  // never destroyed, like the page-locked pool
	static bool enabled() {
		if (getenv("URMAPX_NO_LANE_POOL")) return false;
		for (char **e = environ; e && *e; ++e)
			if (!strncmp(*e, "URMAPX_TEST_", 12) || !strncmp(*e, "URMAPX_DEBUG_", 13)) return false;  // contexts cache what such knobs decide
		return true;
	}
	bool take(const urmapx_index *I, int device, const urmapx_params &P, bool veryfast, bool pair_info, urmapx_ctx *&C, urmapx_text *&T) {
		std::lock_guard<std::mutex> l(m_);
		for (size_t i = 0; i < v_.size(); ++i) {
			const PooledLane &q = v_[i];
			if (q.I == I && q.device == device && q.veryfast == veryfast && q.pair_info == pair_info && q.env == env_knobs() && !memcmp(&q.P, &P, sizeof P)) {
				C = q.C; T = q.T;
				v_.erase(v_.begin() + (long)i);
				return true;
			}
		}
		return false;
	}
	void give(const PooledLane &q) {
		// a kept lane holds 2.5-3 GB of device arrays: it stays only while the device has room to spare -- an eighth of its memory still free
		// with the lane on it (a process that shares the device with other allocators saw the pool's memory as gone)
		size_t free_b = 0, total_b = 0;
		const bool roomy = hipSetDevice(q.device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= total_b / 8;
		if (roomy) {
			std::lock_guard<std::mutex> l(m_);
			if (v_.size() < kMax) { v_.push_back(q); return; }
		}
		destroy(q);
	}
	void purge(const urmapx_index *I) {
		std::vector<PooledLane> out;
		{
			std::lock_guard<std::mutex> l(m_);
			for (size_t i = 0; i < v_.size();)
				if (!I || v_[i].I == I) { out.push_back(v_[i]); v_.erase(v_.begin() + (long)i); }
				else ++i;
		}
		for (const PooledLane &q : out) destroy(q);
	}
	static void destroy(const PooledLane &q) {
		if (q.T) urmapx_text_destroy(q.T);
		if (q.C) urmapx_ctx_destroy(q.C);
	}

private:
	static constexpr size_t kMax = 8;
	std::mutex m_;
	std::vector<PooledLane> v_;
};

// one chunk of the text phase: FASTQ bytes in, SAM bytes out, both page-locked
struct TextJob {
	char *in = nullptr, *out = nullptr;
	size_t in_cap = 0, out_cap = 0, nbytes = 0, nbytes2 = 0;  // pairs: the mate file's chunk is in[...] too, at in2
	char *in2 = nullptr;
	uint64_t file_off = 0, file_off2 = 0;
	urmapx_text_report rep;
	int rc = 0;
	// -tabbedout: the chunk's lines, formatted by the lane's host threads from what urmapx_text_fetch_pairs brings back
	std::string tab;
	std::vector<urmapx_result> tab_res;
	std::vector<urmapx_pair_info> tab_info;
	std::vector<uint32_t> tab_ends, tab_lens2;
	~TextJob() {
		HostPool::get().release(in, in_cap);
		HostPool::get().release(out, out_cap);
	}
	static bool grow(char *&p, size_t &cap, size_t want) {
		if (want <= cap) return true;
		HostPool::get().release(p, cap);
		p = HostPool::get().acquire(want, cap);
		if (!p) cap = 0;
		return p != nullptr;
	}
};

// first record start at or after `from`: a line that begins with '@' whose line after next begins with '+'.  A wrong
// guess cannot pass: the chunk in front would then hold a line count that is not a multiple of four, which the device
// parser reports.  Returns 0 if the window [from, from + 4 MB) shows none.
uint64_t find_record_start(int fd, uint64_t from, uint64_t fsize) {
	std::vector<char> w;
	for (size_t win = 1u << 16; win <= (8u << 20); win *= 4) {
		const size_t len = (size_t)std::min<uint64_t>(win, fsize - from);
		w.resize(len);
		if (!pread_all(fd, w.data(), len, from)) return 0;
		const char *b = w.data(), *e = b + len;
		for (const char *nl = (const char *)memchr(b, '\n', len); nl && nl + 1 < e; nl = (const char *)memchr(nl + 1, '\n', (size_t)(e - nl - 1))) {
			if (nl[1] != '@') continue;
			const char *n1 = (const char *)memchr(nl + 1, '\n', (size_t)(e - nl - 1));
			const char *n2 = n1 && n1 + 1 < e ? (const char *)memchr(n1 + 1, '\n', (size_t)(e - n1 - 1)) : nullptr;
			if (!n2 || n2 + 1 >= e) break;  // the window ends inside this record: look again with a larger one
			if (n2[1] == '+') return from + (uint64_t)(nl + 1 - b);
		}
		if (len < win) return 0;  // the window reached the end of the file
	}
	return 0;
}


// A FASTQ input read front to back as uncompressed bytes: a plain file, or a gzip file (linereader.cpp:14-113 reads .gz
// through zlib) inflated on the fly.  A plain gzip stream is cut into segments that the caller's OpenMP threads inflate side by
// side (pgzip.h, round 5; one zlib stream on one thread until then); a BGZF file (gzip members of <= 64 KB that carry their
// compressed size in a 'BC' extra field, the bgzip / htslib convention) is inflated a batch of blocks at a time by the same threads.
class SeqSource {
public:
	~SeqSource() {
		for (z_stream &z : bz_) inflateEnd(&z);
		if (fd_ >= 0 && own_) ::close(fd_);
	}
	// a descriptor that cannot seek (FIFO, standard input), owned by the caller: plain FASTQ text read front to back
	bool open_pipe(int fd) {
		fd_ = fd; own_ = false; pipe_ = true; gz_ = false;
		return fd >= 0;
	}
	bool is_pipe() const { return pipe_; }
	// regular files only; gz says which kind the name promises (".gz")
	bool open(const char *path, bool gz) {
		fd_ = ::open(path, O_RDONLY);
		struct stat st;
		if (fd_ < 0 || fstat(fd_, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) return false;
		csize_ = (uint64_t)st.st_size;
		gz_ = gz;
		if (!gz_) return true;
		unsigned char h[18];
		if (pread(fd_, h, sizeof h, 0) != (ssize_t)sizeof h || h[0] != 0x1f || h[1] != 0x8b) return false;
		bgzf_ = (h[3] & 4) && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
		if (bgzf_) cbuf_.resize(32u << 20);
		else if (!pg_.open(fd_, csize_)) return false;  // plain gzip: segments of the one stream inflated side by side (pgzip.h)
		return true;
	}
	bool is_gz() const { return gz_; }
	bool returns_whole_rounds() const { return gz_ && !bgzf_ && !pipe_; }  // a plain gzip stream through ParallelGunzip
	bool is_bgzf() const { return bgzf_; }
	bool failed() const { return bad_; }
	uint64_t compressed_size() const { return csize_; }
	// up to cap bytes of the uncompressed stream into dst; 0 = end of input (or failed())
	size_t read(char *dst, size_t cap, int threads) {
		if (cap == 0 || eof_ || bad_) return 0;
		if (pipe_) {
			size_t done = 0;
			while (done < cap) {
				const ssize_t k = ::read(fd_, dst + done, cap - done);
				if (k < 0) { if (errno == EINTR) continue; bad_ = true; break; }
				if (k == 0) { eof_ = true; break; }
				done += (size_t)k;
			}
			return done;
		}
		if (!gz_) {
			const size_t n = (size_t)std::min<uint64_t>(cap, csize_ - cpos_);
			if (n == 0) { eof_ = true; return 0; }
			if (!read_range(fd_, dst, cpos_, n, std::max(1, threads))) { bad_ = true; return 0; }
			cpos_ += n;
			return n;
		}
		if (bgzf_) return read_bgzf(dst, cap, threads);
		const size_t k = pg_.read(dst, cap, gz_threads_ > 0 ? gz_threads_ : threads);
		if (pg_.failed()) bad_ = true;
		if (k == 0) eof_ = true;
		return k;
	}
	// plain gzip: the inflater is what the run waits for -- it may use more threads than the readers of a plain file get
	void set_gz_threads(int t) { gz_threads_ = t; }
	uint64_t gz_parallel_bytes() const { return pg_.parallel_bytes(); }

private:
	bool refill() {  // more compressed bytes behind what cbuf_ still holds
		if (chave_ > cbeg_ && cbeg_ > 0) memmove(cbuf_.data(), cbuf_.data() + cbeg_, chave_ - cbeg_);
		chave_ -= cbeg_; cbeg_ = 0;
		bool got = false;
		while (chave_ < cbuf_.size() && cpos_ < csize_) {
			const ssize_t k = pread(fd_, cbuf_.data() + chave_, cbuf_.size() - chave_, (off_t)cpos_);
			if (k <= 0) { bad_ = true; return false; }
			chave_ += (size_t)k; cpos_ += (uint64_t)k;
			got = true;
		}
		return got;
	}
	size_t read_bgzf(char *dst, size_t cap, int threads) {
		struct Blk { size_t in, in_len, out, out_len; uint32_t crc; };
		std::vector<Blk> blks;
		size_t out = 0;
		for (;;) {
			if (chave_ - cbeg_ < 18 + 8 && !refill() && chave_ == cbeg_) { eof_ = true; break; }
			if (chave_ - cbeg_ < 18 + 8) { bad_ = true; break; }
			const uint8_t *h = cbuf_.data() + cbeg_;
			if (h[0] != 0x1f || h[1] != 0x8b || !(h[3] & 4) || h[12] != 'B' || h[13] != 'C') { bad_ = true; break; }
			const size_t bsize = (size_t)(h[16] | (h[17] << 8)) + 1;
			if (bsize < 26) { bad_ = true; break; }
			if (chave_ - cbeg_ < bsize) {
				if (!blks.empty()) break;  // inflate what is complete first
				if (!refill() || chave_ - cbeg_ < bsize) { bad_ = true; break; }
				continue;
			}
			const uint8_t *tl = cbuf_.data() + cbeg_ + bsize - 4;
			const size_t isize = (size_t)tl[0] | ((size_t)tl[1] << 8) | ((size_t)tl[2] << 16) | ((size_t)tl[3] << 24);
			if (isize > 65536) { bad_ = true; break; }
			if (out + isize > cap) break;
			const uint32_t crc = (uint32_t)tl[-4] | ((uint32_t)tl[-3] << 8) | ((uint32_t)tl[-2] << 16) | ((uint32_t)tl[-1] << 24);
			blks.push_back(Blk{cbeg_ + 18, bsize - 26, out, isize, crc});
			out += isize;
			cbeg_ += bsize;
		}
		if (bad_) return 0;
		if (threads < 1) threads = 1;
		if ((int)bz_.size() < threads) {
			const size_t old = bz_.size();
			bz_.resize((size_t)threads);
			for (size_t i = old; i < bz_.size(); ++i) {
				memset(&bz_[i], 0, sizeof(z_stream));
				if (inflateInit2(&bz_[i], -15) != Z_OK) { bad_ = true; return 0; }
			}
		}
		std::atomic<bool> ok{true};
#pragma omp parallel for schedule(dynamic, 16) num_threads(threads)
		for (long i = 0; i < (long)blks.size(); ++i) {
			z_stream &z = bz_[(size_t)omp_get_thread_num()];
			const Blk &b = blks[(size_t)i];
			if (b.out_len == 0) continue;
			inflateReset(&z);
			z.next_in = cbuf_.data() + b.in; z.avail_in = (uInt)b.in_len;
			z.next_out = (Bytef *)dst + b.out; z.avail_out = (uInt)b.out_len;
			if (inflate(&z, Z_FINISH) != Z_STREAM_END || z.avail_out != 0) ok.store(false);
			// the member's CRC-32, as zlib's gzread checks it for the reference (a raw inflate does not): round 5
			else if (crc32_fast((const uint8_t *)dst + b.out, b.out_len) != b.crc) ok.store(false);
		}
		if (!ok) { bad_ = true; return 0; }
		return out;
	}
	int fd_ = -1;
	bool gz_ = false, bgzf_ = false, eof_ = false, bad_ = false, pipe_ = false, own_ = true;
	uint64_t csize_ = 0, cpos_ = 0;  // compressed (or plain) file: size, next byte to fetch
	std::vector<uint8_t> cbuf_;
	size_t cbeg_ = 0, chave_ = 0;
	ParallelGunzip pg_;
	int gz_threads_ = 0;
	std::vector<z_stream> bz_;
};

// start of the last record of b[0, n) whose first three lines lie inside the buffer: a line that begins with '@' whose line
// after next begins with '+' (only label and quality lines can begin with '@', and two lines after a quality line come
// bases).  0: none in sight (n holds less than one such record: the caller reads more).
size_t last_record_start(const char *b, size_t n) {
	for (size_t win = 1u << 16;; win *= 8) {
		const size_t lo = n > win ? n - win : 0;
		const char *p = b + lo, *e = b + n;
		if (lo) {  // to the first line start at or behind lo
			p = (const char *)memchr(p, '\n', (size_t)(e - p));
			if (!p) { if (lo == 0) return 0; continue; }
			++p;
		}
		size_t best = 0;
		while (p < e) {
			const char *n1 = (const char *)memchr(p, '\n', (size_t)(e - p));
			if (!n1) break;
			if (*p == '@') {
				const char *n2 = n1 + 1 < e ? (const char *)memchr(n1 + 1, '\n', (size_t)(e - n1 - 1)) : nullptr;
				if (n2 && n2 + 1 < e && n2[1] == '+') best = (size_t)(p - b);
			}
			p = n1 + 1;
		}
		if (best) return best;
		if (lo == 0) return 0;
	}
}

}  // namespace

namespace {
// One shard of a sharded run (urmapx_map_options.sam_shards): the records of bytes [lo, hi) of the (plain, seekable) input
// file(s), cut at record starts; the SAM header only in the first shard.
struct InputRange {
	// out: when this pipeline's clock started (contexts made, files open) and stopped, on the steady clock -- the wall time of a
	// sharded run is first start .. last stop, with the set-up outside as in a run of one pipeline
	mutable double t_begin = 0, t_end = 0;
	bool on = false;
	uint64_t lo[2] = {0, 0}, hi[2] = {0, 0};
	uint64_t lines_before = 0;  // lines of each file in front of lo (they name the line in the reader's messages)
	// single-end shards: the lines in front of lo are counted only if a message needs a line number (lines_before stays 0 until then)
	std::function<uint64_t()> lazy_lines;
	bool header = true;
};

// number of '\n' in bytes [from, to) of fd, by all threads
// per_piece (optional): the count of every 8 MB piece, for line_offsets below
uint64_t count_newlines(int fd, uint64_t from, uint64_t to, int threads, std::vector<uint64_t> *per_piece = nullptr) {
	if (to <= from) return 0;
	const uint64_t piece = 8u << 20;
	const uint64_t np = (to - from + piece - 1) / piece;
	if (per_piece) per_piece->assign((size_t)np, 0);
	uint64_t total = 0;
#pragma omp parallel num_threads(threads) reduction(+ : total)
	{
	std::vector<char> buf((size_t)std::min<uint64_t>(piece, to - from));  // one buffer per thread, not per piece
#pragma omp for schedule(dynamic, 1)
	for (int64_t k = 0; k < (int64_t)np; ++k) {
		const uint64_t a = from + (uint64_t)k * piece, b = std::min(to, a + piece);
		size_t have = 0;
		while (a + have < b) {
			const ssize_t r = pread(fd, buf.data() + have, (size_t)(b - a - have), (off_t)(a + have));
			if (r <= 0) break;
			have += (size_t)r;
		}
		const uint64_t n = count_nl(buf.data(), buf.data() + have);
		total += n;
		if (per_piece) (*per_piece)[(size_t)k] = n;
	}
	}
	return total;
}

// offset of the byte behind the `lines`-th '\n' of fd at or after `from` (`fsize` if the file has fewer)
uint64_t skip_lines(int fd, uint64_t from, uint64_t fsize, uint64_t lines) {
	std::vector<char> buf(8u << 20);
	uint64_t at = from;
	while (lines && at < fsize) {
		const ssize_t r = pread(fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), fsize - at), (off_t)at);
		if (r <= 0) return fsize;
		const char *c = buf.data(), *e = c + r;
		while (lines && c < e) {
			const char *nl = (const char *)memchr(c, '\n', (size_t)(e - c));
			if (!nl) { c = e; break; }
			--lines;
			c = nl + 1;
		}
		at += (uint64_t)(c - buf.data());
	}
	return lines ? fsize : at;
}

// offsets of the bytes behind the targets[i]-th '\n' of fd (`fsize` where the file has fewer), targets ascending: the pieces' line
// counts by all threads, then one scan inside the piece each target falls in (the mates' file of a sharded paired run used to be
// walked by one thread from its start to the last cut)
std::vector<uint64_t> line_offsets(int fd, uint64_t fsize, const std::vector<uint64_t> &targets, int threads) {
	std::vector<uint64_t> per, out(targets.size(), fsize);
	count_newlines(fd, 0, fsize, threads, &per);
	const uint64_t piece = 8u << 20;
	uint64_t before = 0;
	size_t k = 0;
	for (size_t i = 0; i < targets.size(); ++i) {
		if (targets[i] == 0) { out[i] = 0; continue; }
		while (k < per.size() && before + per[k] < targets[i]) before += per[k++];
		if (k == per.size()) break;  // fewer lines than asked for: fsize
		out[i] = skip_lines(fd, (uint64_t)k * piece, fsize, targets[i] - before);
	}
	return out;
}

// Where a device hangs: its PCI function's NUMA node (/sys/bus/pci/devices/<bus id>/numa_node) and that node's CPUs that this process
// may use.  On an 8-GPU node the devices sit behind two sockets: a lane thread that drives device g -- it fills and drains the
// page-locked chunk buffers that cross PCIe -- runs on g's socket, and so do the reader and the writer of a shard whose devices are
// all there.  ok == false (no such file, node -1 as on one-socket boxes and in most VMs, or none of the node's CPUs
// allowed): nothing is pinned.
struct DevicePlace {
	int node = -1;
	cpu_set_t cpus;
	bool ok = false;
};
DevicePlace place_of_device(int device) {
	DevicePlace P;
	CPU_ZERO(&P.cpus);
	char bus[64] = {0};
	if (getenv("URMAPX_NO_NUMA_PIN") || hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) return P;
	for (char *c = bus; *c; ++c) *c = (char)tolower((unsigned char)*c);
	const char *forced = getenv("URMAPX_TEST_NUMA_NODE");  // test aid: pretend every device hangs off this node
	if (forced) P.node = atoi(forced);
	else {
		FILE *f = fopen((std::string("/sys/bus/pci/devices/") + bus + "/numa_node").c_str(), "r");
		if (!f) return P;
		if (fscanf(f, "%d", &P.node) != 1) P.node = -1;
		fclose(f);
	}
	if (P.node < 0) return P;
	FILE *f = fopen(("/sys/devices/system/node/node" + std::to_string(P.node) + "/cpulist").c_str(), "r");
	if (!f) return P;
	char list[4096] = {0};
	const bool got = fgets(list, sizeof list, f) != nullptr;
	fclose(f);
	if (!got) return P;
	cpu_set_t allowed;
	CPU_ZERO(&allowed);
	if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return P;
	for (const char *c = list; *c && *c != '\n';) {  // "0-63,128-191"
		char *e;
		const long a = strtol(c, &e, 10);
		long b = a;
		if (e == c) break;
		if (*e == '-') { c = e + 1; b = strtol(c, &e, 10); }
		for (long k = a; k <= b && k < CPU_SETSIZE; ++k)
			if (CPU_ISSET((int)k, &allowed)) CPU_SET((int)k, &P.cpus);
		c = *e == ',' ? e + 1 : e;
	}
	P.ok = CPU_COUNT(&P.cpus) > 0;
	return P;
}
// Idle OpenMP workers must sleep, not spin: the reader, the writer, every lane and the caller each have a team of their own, and libomp's
// default keeps a team's workers spinning for 200 ms behind every parallel region (KMP_BLOCKTIME).  Three or four teams of 16 spinning
// threads on a host that grants the process 16 CPUs (a cgroup quota, as on the GPU boxes) get the whole process throttled: the lanes' host
// threads stall between their launches and a run takes three times as long -- seen in half of the bench runs of round 5 (the command line
// has always set OMP_WAIT_POLICY=passive for this; a library call cannot count on its caller's environment).  Per thread: it applies to the
// teams this thread starts.
// kmp_set_blocktime is libomp's (the runtime hipcc links); under another OpenMP runtime -- the sanitizer builds use g++ -- idle workers
// are the caller's business (OMP_WAIT_POLICY=passive, which the command line and bench.py set anyway).
#ifdef KMP_VERSION_MAJOR
inline void omp_workers_sleep_when_idle() { kmp_set_blocktime(0); }
inline int omp_idle_blocktime() { return kmp_get_blocktime(); }
inline void omp_set_idle_blocktime(int ms) { kmp_set_blocktime(ms); }
#else
inline void omp_workers_sleep_when_idle() {}
inline int omp_idle_blocktime() { return 0; }
inline void omp_set_idle_blocktime(int) {}
#endif

// the calling thread (and the OpenMP team it starts later) onto a device's socket; false: left where it was
bool pin_to(const DevicePlace &P) { return P.ok && sched_setaffinity(0, sizeof P.cpus, &P.cpus) == 0; }
// A pipeline thread that pinned itself hands its OpenMP workers back unpinned: the workers of its team inherited its
// narrowed mask when they were made, libomp returns them to a pool the CALLER's later parallel regions draw from, and those would
// then run on one socket.  Run by the pinned thread as its last act: every thread of its team takes the mask the caller had.
struct Unpin {
	bool was_pinned;
	const cpu_set_t &caller_mask;
	int team;
	~Unpin() {
		if (!was_pinned) return;
#pragma omp parallel num_threads(team > 0 ? team : 1)
		(void)sched_setaffinity(0, sizeof caller_mask, &caller_mask);
	}
};
void omp_team(int n) { omp_workers_sleep_when_idle(); omp_set_num_threads(n); }
void say(char *err, size_t errcap, const std::string &s) {
	if (err && errcap) snprintf(err, errcap, "%s", s.c_str());
}
// the table per reference of this thread's last run with depth_out (urmapx_map_depth_summary)
std::string &depth_summary() {
	static thread_local std::string table;
	return table;
}
// host threads for FASTQ parsing and SAM formatting (the mapping itself runs on the GPU)
int host_threads_of(const urmapx_map_options &o) {
	return o.host_threads > 0 ? o.host_threads : std::min(16, std::max(1, (int)std::thread::hardware_concurrency()));
}
// URMAPX_FORCE_DEVICE=d (test aid): every lane runs on physical device d, so that the N-device code path can be
// exercised on a machine with one GPU
int phys_device(const urmapx_map_options &o, int g) {
	const char *forced = getenv("URMAPX_FORCE_DEVICE");
	return forced ? atoi(forced) : o.first_gpu + g;
}
std::string shard_name(const char *path, int s) { return std::string(path) + "." + std::to_string(s); }
void create_empty(const std::string &path) { if (FILE *f = fopen(path.c_str(), "wb")) fclose(f); }
bool is_gz_name(const char *path) { const size_t l = strlen(path); return l > 3 && !strcmp(path + l - 3, ".gz"); }
// a non-empty regular file that is neither .gz nor standard input: its descriptor and size, else -1
int open_plain(const char *path, uint64_t &size) {
	if (is_gz_name(path) || !strcmp(path, "-")) return -1;
	const int fd = open(path, O_RDONLY);
	struct stat st;
	if (fd >= 0 && (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0)) { close(fd); return -1; }
	if (fd >= 0) size = (uint64_t)st.st_size;
	return fd;
}
// '\n' count of each of `threads` slices of p[0, n), and their sum
size_t count_lines(const char *p, size_t n, int threads, std::vector<size_t> &per) {
	per.assign((size_t)threads, 0);
#pragma omp parallel for schedule(static, 1) num_threads(threads)
	for (int t = 0; t < threads; ++t) per[(size_t)t] = count_nl(p + part(n, t, threads), p + part(n, t + 1, threads));
	size_t lines = 0;
	for (size_t k : per) lines += k;
	return lines;
}
// offset behind the `lines`-th '\n' of p[0, n), given count_lines' counts of its slices; 0: p holds fewer (or none is asked for)
size_t nth_line_end(const char *p, size_t n, const std::vector<size_t> &per, size_t lines) {
	const int T = (int)per.size();
	size_t cum = 0;
	for (int t = 0; t < T && lines > 0; ++t) {
		if (cum + per[(size_t)t] >= lines) {  // the chunk ends in this slice: walk to its last '\n'
			const char *c = p + part(n, t, T), *e = p + part(n, t + 1, T);
			for (size_t need = lines - cum; need; --need) c = (const char *)memchr(c, '\n', (size_t)(e - c)) + 1;
			return (size_t)(c - p);
		}
		cum += per[(size_t)t];
	}
	return 0;
}
// a larger page-locked buffer for the job's input, holding the first `keep` bytes and the `keep2` bytes at `at2` of the old one
bool regrow(TextJob &j, size_t want, size_t keep, size_t at2 = 0, size_t keep2 = 0) {
	size_t ncap = 0;
	char *nb = HostPool::get().acquire(want, ncap);
	if (!nb) return false;
	if (keep) memcpy(nb, j.in, keep);
	if (keep2) memcpy(nb + at2, j.in + at2, keep2);
	HostPool::get().release(j.in, j.in_cap);
	j.in = nb; j.in_cap = ncap;
	return true;
}
// The mate file's chunk of a text job as the reader cuts it: it lies in the job's buffer behind the first file's `keep` bytes, from
// `pad` on (a multiple of 4096)
struct MateChunk {
	TextJob &j;
	size_t keep, pad;
	size_t have = 0, n2 = 0;  // mate bytes read into the buffer; of them the chunk's: as many lines as the first file's chunk holds
	bool found = false, give_up = false;
	char *dst() const { return j.in + pad; }
	// the mate chunk outgrew the buffer (its records are longer than the first file's were so far): a larger one, with what has been read
	bool grow(size_t room) { return regrow(j, pad + room, keep, pad, have); }
	void end_at(size_t n) { n2 = n; found = true; }
	// the cut stands: the job gets the chunk, and the next buffer is sized by the ratio seen
	void hand_to_job(double &bytes2_per_byte1) {
		j.in2 = dst(); j.nbytes2 = n2;
		if (keep && n2) bytes2_per_byte1 = (double)n2 / (double)keep;
	}
};
// the fields of a report that add up over the shards of a sharded run
using Rep = urmapx_map_report;
constexpr uint64_t Rep::*kReportCounts[] = {&Rep::reads, &Rep::mapped_q, &Rep::mapped_lowq, &Rep::unmapped, &Rep::unsupported, &Rep::input_bytes, &Rep::sam_text_bytes, &Rep::sam_file_bytes};
constexpr double Rep::*kReportTimes[] = {&Rep::parse_s, &Rep::gpu_s, &Rep::format_s, &Rep::write_s, &Rep::dev_h2d_s, &Rep::dev_parse_s, &Rep::dev_map_s, &Rep::dev_format_s,
	&Rep::dev_d2h_s, &Rep::dev_map_search_s, &Rep::dev_map_dp_s, &Rep::map_enqueue_s};

// One run of one pipeline (urmapx_map_files, or one shard of it): what its stages share.  open() fills it, the text phase and the host phase
// run on it one after the other, finish() ends the files and reports.  While a phase's threads run, a member without a note is only read.
struct Run {
	urmapx_index *const I;
	const urmapx_map_options &opt;
	const InputRange &range;
	const char *const fastq1, *const fastq2, *const samout, *const tabout;
	// constants derived from the options
	const bool paired = fastq2 != nullptr;
	const int gpus = opt.gpus > 0 ? opt.gpus : 1, streams = opt.streams > 0 ? opt.streams : 2, n_lanes = gpus * streams;
	const int host_threads = host_threads_of(opt);
	const uint32_t batch = opt.batch ? opt.batch : (1u << 18);
	const unsigned minq = paired ? opt.minq : 10;  // only cmd_map2 reads -minq (map2.cpp:76); -map keeps State1::m_Minq = 10
	const bool have_sam = samout != nullptr;
	const bool bam = opt.bam != 0 && have_sam;  // -bamout: BAM records where the SAM text was, always inside BGZF members
	const bool sort = opt.bam_sort != 0 && bam;  // -sort: the lanes' raw records are kept in host memory; finish() sorts them and writes samout and its index
	const bool bgzf = (opt.bgzf != 0 || bam) && have_sam && !sort;
	// -tags / -rg: the optional fields of the records (map_files_entry has checked both); rg_id: the ID: value of the @RG line
	const unsigned tags = have_sam ? opt.tags & URMAPX_TAG_ALL : 0u;
	const char *const rg_line = have_sam ? opt.read_group : nullptr;
	std::string rg_id;
	bool tagged() const { return tags != 0 || rg_line != nullptr; }
	const bool pool_lanes = LanePool::enabled(), lane_veryfast = paired && opt.veryfast, lane_pair_info = paired && tabout != nullptr;
	urmapx_params P;
	// one replica of the index per device (uploaded concurrently), K mapping contexts on each
	std::vector<urmapx_index *> replicas;
	std::vector<urmapx_ctx *> ctxs;
	std::vector<urmapx_text *> texts;  // a lane's text stage: from the pool, or made by the lane's thread -- [l] is written by text lane l
	bool run_ok = false;  // set at the end of a run without failure: only then are the lanes worth keeping
	// where each device hangs (NUMA node of its PCI function): lane threads run there; a pipeline whose devices share one node -- every
	// shard of a sharded run on a two-socket node -- has its reader and writer there too
	std::vector<DevicePlace> places;
	bool one_node = false;
	cpu_set_t caller_mask;
	// this is a library call: the caller's OpenMP setting comes back at the end
	// (the calling thread's block time comes back too -- kmp_set_blocktime(0) applies to the teams THIS thread starts later)
	const int omp_threads_before = omp_get_max_threads(), omp_blocktime_before = omp_idle_blocktime();
	FileSink sink;
	std::unique_ptr<FILE, int (*)(FILE *)> ftab{nullptr, fclose};  // -tabbedout (outfiles.cpp:7-12): State2::OutputTab2's line per pair; only -map2 writes it
	FastqReader rd, rd2;  // the host reader's and the mate reader's (host phase)
	Failure fail;
	Trace trace;
	Clock::time_point t1;
	// The running totals, as they are reported.  Written while threads run by:
	//   reads .. unsupported, input_bytes, sam_text_bytes, dev_*_s, map_enqueue_s   the text writer; the host formatter
	//   sam_file_bytes   the same two: it is the offset in samout at which the next piece goes (the header's size before the first)
	//   parse_s          the text reader; the host reader
	//   write_s          the text writer; the flusher
	//   gpu_s            every lane, under lane_time_lock
	//   format_s         the text lanes (tab lines), under lane_time_lock; the host formatter
	urmapx_map_report rep{};
	std::mutex lane_time_lock;
	~Run() {
		close();
		omp_set_num_threads(omp_threads_before);
		omp_set_idle_blocktime(omp_blocktime_before);
	}
	int phys(int g) const { return phys_device(opt, g); }
	int failed(int rc, std::string &msg, const std::string &why) const { msg = why; return rc; }
	void add_lane_time(double Rep::*stage, Clock::time_point since) {
		std::lock_guard<std::mutex> g(lane_time_lock);
		rep.*stage += secs(since, now());
	}
	void cannot_write_sam() { fail.raise(URMAPX_E_IO, std::string("Error writing ") + samout); }
	int open(std::string &msg) {
		if (gpus > 64 || streams > 8) return failed(URMAPX_E_ARG, msg, "gpus must be 1..64, streams 1..8");
		int rc = urmapx_params_for_method((opt.veryfast && !paired) ? 7 : 6, &P);  // -map2 always uses method 6 (map2.cpp:15-16)
		if (rc) return rc;
		if (rg_line) {
			char id[1024], why[256];
			if (urmapx_read_group_id(rg_line, nullptr, 0, id, sizeof id, why, sizeof why)) return failed(URMAPX_E_ARG, msg, why);
			rg_id = id;
		}
		replicas.assign((size_t)gpus, nullptr);
		ctxs.assign((size_t)n_lanes, nullptr);
		texts.assign((size_t)n_lanes, nullptr);
		std::vector<int> rcs((size_t)gpus, 0);
		std::vector<std::thread> up;
		for (int g = 0; g < gpus; ++g)
			up.emplace_back([&, g] {
				if (g == 0) { rcs[0] = urmapx_index_upload(I, phys(0)); replicas[0] = I; }
				else rcs[(size_t)g] = urmapx_index_replicate(I, phys(g), &replicas[(size_t)g]);
			});
		for (auto &t : up) t.join();
		for (int g = 0; g < gpus; ++g)
			if (rcs[(size_t)g]) return failed(rcs[(size_t)g], msg, std::string("Uploading index to the GPU: ") + urmapx_strerror(rcs[(size_t)g]));
		for (int l = 0; l < n_lanes; ++l) {
			if (pool_lanes && l % gpus == 0 && LanePool::get().take(I, phys(0), P, lane_veryfast, lane_pair_info, ctxs[(size_t)l], texts[(size_t)l])) continue;
			rc = urmapx_ctx_create(replicas[(size_t)(l % gpus)], phys(l % gpus), &P, &ctxs[(size_t)l]);
			if (!rc && paired && opt.veryfast) rc = urmapx_ctx_set_pe_veryfast(ctxs[(size_t)l], 1);
			if (!rc && paired && tabout) rc = urmapx_ctx_set_pair_info(ctxs[(size_t)l], 1);
			if (rc) return failed(rc, msg, std::string("Creating mapping context: ") + urmapx_strerror(rc));
		}
		places.resize((size_t)gpus);
		for (int g = 0; g < gpus; ++g) places[(size_t)g] = place_of_device(phys(g));
		one_node = places[0].ok;
		for (int g = 1; g < gpus; ++g) one_node = one_node && places[(size_t)g].ok && places[(size_t)g].node == places[0].node;
		std::string placement;
		for (int g = 0; g < gpus; ++g)
			placement += (g ? " gpu" : "gpu") + std::to_string(phys(g)) + (places[(size_t)g].ok ? "@node" + std::to_string(places[(size_t)g].node) : std::string("@any"));
		placement += one_node ? "; reader+writer@node" + std::to_string(places[0].node) : std::string("; reader+writer@any");
		snprintf(rep.placement, sizeof rep.placement, "%s", placement.c_str());
		omp_team(host_threads);
		CPU_ZERO(&caller_mask);
		(void)sched_getaffinity(0, sizeof caller_mask, &caller_mask);
		rep.host_threads = host_threads; rep.lanes = n_lanes; rep.write_threads = 1; rep.shards = 1;
		if (samout) {
			if (sort) {  // (the index needs a file name to sit beside)
				struct stat st;
				if (stat(samout, &st) == 0 && !S_ISREG(st.st_mode)) return failed(URMAPX_E_ARG, msg, std::string("bam_sort needs a regular file, not ") + samout);
			}
			if (opt.discard_sam) sink.open_discard();
			else if (!sink.open(samout)) return failed(URMAPX_E_IO, msg, std::string("Cannot create ") + samout);
			if (sort) sink.keep_in_memory();  // (the header block is made in write_sorted; the records start at offset 0 of the kept bytes)
			else if (range.header || bam) {  // (every shard of a BAM run is a BAM file: each has the header block)
				std::string hdr;
				if (bam) append_bam_header(hdr, I, opt.cmdline, false, rg_line);
				else append_sam_header_text(hdr, I, opt.cmdline, rg_line);
				rep.sam_text_bytes += hdr.size();
				if (bgzf && !bgzf_members(hdr)) return failed(URMAPX_E_NOMEM, msg, "out of memory");  // (members of its own: the chunks' come from the device)
				if (!sink.write_at(hdr.data(), hdr.size(), 0, 1)) return failed(URMAPX_E_IO, msg, std::string("Cannot write ") + samout);
				rep.sam_file_bytes = hdr.size();
			}
		}
		snprintf(rep.medium, sizeof rep.medium, "%s", have_sam ? sink.medium() : "none");
		if (tabout) {
			ftab.reset(fopen(tabout, "wb"));
			if (!ftab) return failed(URMAPX_E_IO, msg, std::string("Cannot create ") + tabout);
		}
		std::string e;
		if (!rd.open(fastq1, e) || (paired && !rd2.open(fastq2, e))) return failed(URMAPX_E_IO, msg, e);
		if (range.on) {  // the host reader, should it be needed, starts and stops where the shard does
			if (!rd.resume_at(range.lo[0], range.lines_before) || (paired && !rd2.resume_at(range.lo[1], range.lines_before)))
				return failed(URMAPX_E_IO, msg, std::string("Cannot read a part of ") + fastq1);
			rd.set_limit(range.hi[0]);
			if (paired) rd2.set_limit(range.hi[1]);
			if (range.lazy_lines) rd.set_lazy_line_base(range.lazy_lines);
		}
		t1 = now();
		trace.t0 = t1;
		return 0;
	}
	// the tab file, then the lanes -- back to the pool or destroyed -- and only then the other devices' replicas
	void close() {
		ftab.reset();
		for (size_t l = 0; l < ctxs.size(); ++l) {
			urmapx_ctx *C = ctxs[l];
			urmapx_text *T = texts[l];
			// (a lane of the caller's own index only: the other devices' replicas are closed below.  set_deferred refuses while a text is on its way)
			if (C && pool_lanes && run_ok && l % (size_t)gpus == 0 && replicas[0] == I && (!T || urmapx_text_set_deferred(T, 0) == URMAPX_OK))
				LanePool::get().give(PooledLane{I, phys(0), P, lane_veryfast, lane_pair_info, C, T, env_knobs()});
			else LanePool::destroy(PooledLane{I, 0, P, false, false, C, T, 0});
		}
		for (size_t g = 1; g < replicas.size(); ++g) urmapx_index_close(replicas[g]);
		ctxs.clear(); texts.clear(); replicas.clear();  // (the destructor's pass finds nothing)
	}
	// ---- bam_sort: the kept records (rep.sam_file_bytes of them, in input order) into coordinate order, then samout -- header block with
	// the @HD line in a member of its own, the sorted stream, the end-of-file member -- and samout.bai; under depth_out the bedGraph file, under stats_out the statistics', under vcf_out the pileup's ----
	// What the parts of write_sorted hand on.  Both results are freed on every way out; where the library has freed and zeroed them
	// already (a call that failed) the frees find null pointers
	struct Sorted {
		std::string hdr;  // the header block, as BGZF members
		uint64_t n_bytes = 0;  // of the kept records
		uint32_t n_ref = 0;
		urmapx_bam_sort_result S;
		urmapx_markdup_stats M;
		urmapx_depth_result D;
		urmapx_stats_result T;
		urmapx_pileup_result V;
		std::vector<const char *> ref_names;  // depth_out, stats_out, vcf_out: the names and lengths of the @SQ lines
		std::vector<uint32_t> ref_lens;
		Sorted() { memset(&S, 0, sizeof S); memset(&M, 0, sizeof M); memset(&D, 0, sizeof D); memset(&T, 0, sizeof T); memset(&V, 0, sizeof V); }
		Sorted(const Sorted &) = delete;
		~Sorted() { urmapx_bam_sort_free(&S); urmapx_depth_free(&D); urmapx_stats_free(&T); urmapx_pileup_free(&V); }
	};
	static bool host_sort() { return getenv("URMAPX_HOST_TEXT") || getenv("URMAPX_HOST_SORT"); }
	void write_sorted() {
		const auto t0 = now();
		Sorted W;
		W.n_bytes = rep.sam_file_bytes;
		W.n_ref = urmapx_index_seq_count(I);
		if (!sorted_header(W.hdr)) return;
		if (const int rc = sort_kept(W)) { refuse_sort(rc, W); return; }
		sink.drop_kept();
		sink.write_through();
		const double bam_s = write_bam_and_bai(W);
		const double sorted_s = rep.sort_s = secs(t0, now());
		double bed_s = 0, stats_file_s = 0, vcf_file_s = 0;
		if (opt.depth_out) bed_s = write_depth(W);
		if (opt.stats_out) stats_file_s = write_stats(W);
		if (opt.vcf_out) vcf_file_s = write_vcf(W);
		if (opt.depth_out || opt.stats_out || opt.vcf_out) rep.sort_s = secs(t0, now());
		report_sorted(W, sorted_s, bam_s, bed_s, stats_file_s, vcf_file_s);
		trace.add("sort", -1, 0, t0);
	}
	bool sorted_header(std::string &hdr) {
		append_bam_header(hdr, I, opt.cmdline, true, rg_line);
		rep.sam_text_bytes += hdr.size();
		if (!bgzf_members(hdr)) { fail.raise(URMAPX_E_NOMEM, "out of memory"); return false; }
		return true;
	}
	// The sort, on the first device.  Planned -- sort_mem, depth_out, stats_out or vcf_out (all three are taken on the way: include/urmapx.h
	// "Depth", "Stats", "Pileup") or the test knob that forces partitions --: one call, which plans from the budget and streams where it must
	// (urmapx_bam_sort_with; with none of the results that is urmapx_bam_sort_external), and nothing else is tried.  Else in core, and if the records do not fit,
	// planned from the memory that is free.  Where the device is full of lanes, this run's and the pool's go first (the mapping is over)
	// and the same call is made once more.  Under URMAPX_HOST_TEXT / URMAPX_HOST_SORT the host's sort, once
	int sort_kept(Sorted &W) {
		const std::vector<uint64_t> starts = sink.kept_starts();
		const void *const rec = sink.kept();
		const size_t n_bytes = (size_t)W.n_bytes, in_front = W.hdr.size();
		urmapx_markdup_stats *const md = opt.markdup ? &W.M : nullptr;
		urmapx_depth_result *const depth = opt.depth_out ? &W.D : nullptr;
		const urmapx_depth_opts dopts{opt.depth_mapq};
		urmapx_stats_result *const stats = opt.stats_out ? &W.T : nullptr;
		urmapx_pileup_result *const pileup = opt.vcf_out ? &W.V : nullptr;
		const urmapx_pileup_opts popts{opt.vcf_mapq, opt.vcf_baseq, opt.vcf_min_alt, opt.vcf_min_pct};
		for (uint32_t r = 0; (depth || stats || pileup) && r < W.n_ref; ++r) {
			W.ref_names.push_back(urmapx_index_label(I, r));
			W.ref_lens.push_back(urmapx_index_seq_length(I, r));
		}
		// (the pileup's bases: the index's store, in place where it is resident on the sort's device, else fetched once)
		const urmapx_bam_sort_extras extras{md, &dopts, W.ref_names.data(), W.ref_lens.data(), depth, stats, opt.cmdline, &popts, nullptr, I, pileup, opt.cmdline};
		if (host_sort()) return urmapx_bam_sort_with_host(rec, n_bytes, W.n_ref, in_front, starts.data(), starts.size(), &extras, &W.S);
		auto planned_sort = [&]() { return urmapx_bam_sort_with(phys(0), opt.sort_mem, rec, n_bytes, W.n_ref, in_front, starts.data(), starts.size(), &extras, &W.S); };
		auto in_core = [&]() {
			return md ? urmapx_bam_sort_markdup(phys(0), rec, n_bytes, W.n_ref, in_front, starts.data(), starts.size(), md, &W.S)
			          : urmapx_bam_sort(phys(0), rec, n_bytes, W.n_ref, in_front, starts.data(), starts.size(), &W.S);
		};
		const bool planned = depth || stats || pileup || opt.sort_mem != 0 || getenv("URMAPX_TEST_SORT_PARTITION");
		int rc = planned ? planned_sort() : in_core();
		if (rc == URMAPX_E_NOMEM) {
			close();
			LanePool::get().purge(nullptr);
			rc = planned ? planned_sort() : in_core();
		}
		if (rc == URMAPX_E_NOMEM && !planned) rc = planned_sort();
		return rc;
	}
	// why the sort did not run: the device sorts' out-of-memory with the least budget that would do, the depth's references, or the code
	void refuse_sort(int rc, const Sorted &W) {
		if (rc == URMAPX_E_NOMEM && !host_sort() && opt.vcf_out) {
			if (W.V.least_budget)
				fail.raise(rc, "bam_sort with vcf_out: the pileup's counters (16 bytes a reference base), the sort's arrays, its staging buffers and one slice need at least " +
				                   std::to_string(W.V.least_budget) + " bytes on the device" +
				                   (opt.sort_mem ? ", " + std::to_string(opt.sort_mem) + " were given (sort_mem)" : std::string(", fewer are free")));
			else
				fail.raise(rc, "bam_sort with vcf_out: out of device memory");
		} else if (rc == URMAPX_E_NOMEM && !host_sort() && !opt.depth_out && opt.stats_out) {
			if (W.T.least_budget)
				fail.raise(rc, "bam_sort with stats: the statistics' tables, the sort's arrays, its staging buffers and one slice need at least " +
				                   std::to_string(W.T.least_budget) + " bytes on the device" +
				                   (opt.sort_mem ? ", " + std::to_string(opt.sort_mem) + " were given (sort_mem)" : std::string(", fewer are free")));
			else
				fail.raise(rc, "bam_sort with stats: out of device memory");
		} else if (rc == URMAPX_E_NOMEM && !host_sort() && opt.depth_out) {
			if (W.D.least_budget)
				fail.raise(rc, "bam_sort with depth: the depth's counters, the sort's arrays, its staging buffers and one slice need at least " +
				                   std::to_string(W.D.least_budget) + " bytes on the device" +
				                   (opt.sort_mem ? ", " + std::to_string(opt.sort_mem) + " were given (sort_mem)" : std::string(", fewer are free")));
			else
				fail.raise(rc, "bam_sort with depth: out of device memory");
		} else if (rc == URMAPX_E_NOMEM && !host_sort()) {
			size_t free_b = 0, total_b = 0;
			(void)hipSetDevice(phys(0));
			if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
			const uint64_t have = opt.sort_mem ? opt.sort_mem : free_b > URMAPX_SORT_HEADROOM ? (uint64_t)free_b - URMAPX_SORT_HEADROOM : 1u;
			urmapx_bam_sort_plan plan;
			if (urmapx_bam_sort_plan_for((size_t)W.n_bytes, rep.reads, opt.markdup != 0, have, &plan) == URMAPX_E_NOMEM)
				fail.raise(rc, "bam_sort: the sort's arrays, its staging buffers and one slice need at least " + std::to_string(plan.device_bytes) +
				                   " bytes on the device, " + std::to_string(have) + (opt.sort_mem ? " were given (sort_mem)" : " are free"));
			else
				fail.raise(rc, "bam_sort: out of device memory: the plan takes " + std::to_string(plan.device_bytes) + " bytes, " + std::to_string(free_b) + " are free");
		} else if (rc == URMAPX_E_ARG && opt.depth_out)
			fail.raise(rc, "depth: a reference name that is empty or longer than 255 bytes");
		else if (rc == URMAPX_E_ARG && opt.stats_out)
			fail.raise(rc, "stats: a reference name that is empty or longer than 255 bytes");
		else if (rc == URMAPX_E_ARG && opt.vcf_out)
			fail.raise(rc, "vcf_out: a reference name that is empty or longer than 255 bytes, or an index without its sequences");
		else
			fail.raise(rc, std::string("bam_sort: ") + urmapx_strerror(rc));
	}
	// samout and samout.bai -> the seconds it took
	double write_bam_and_bai(const Sorted &W) {
		const auto tw0 = now();
		const urmapx_bam_sort_result &S = W.S;
		std::string eof;
		(void)bgzf_members(eof, 1);
		const int wt = sink.writer_threads(host_threads);
		if (!sink.write_at(W.hdr.data(), W.hdr.size(), 0, 1) || !sink.write_at((const char *)S.bgzf, S.bgzf_bytes, W.hdr.size(), wt) ||
		    !sink.write_at(eof.data(), eof.size(), W.hdr.size() + S.bgzf_bytes, 1))
			cannot_write_sam();
		rep.sam_file_bytes = W.hdr.size() + S.bgzf_bytes + eof.size();
		const std::string bai = std::string(samout) + ".bai";
		FILE *f = fopen(bai.c_str(), "wb");
		if (!f || fwrite(S.bai, 1, S.bai_bytes, f) != S.bai_bytes) fail.raise(URMAPX_E_IO, "Error writing " + bai);
		if (f && fclose(f) != 0) fail.raise(URMAPX_E_IO, "Error writing " + bai);
		const double s = secs(tw0, now());
		rep.write_s += s;
		return s;
	}
	// the bedGraph file, with the writer threads a file of the sink's kind gets; then the summary table and its totals -> the file's seconds
	double write_depth(const Sorted &W) {
		const auto td0 = now();
		const urmapx_depth_result &D = W.D;
		FileSink dsink;
		if (!dsink.open(opt.depth_out) || !dsink.write_at(D.text, D.text_bytes, 0, dsink.writer_threads(host_threads)) || !dsink.finish(D.text_bytes))
			fail.raise(URMAPX_E_IO, std::string("Error writing ") + opt.depth_out);
		const double file_s = secs(td0, now());
		rep.write_s += file_s;
		rep.depth_runs = D.runs;
		std::string &table = depth_summary();
		table = "reference\tlength\treads\tcovered\tpercent\tmean_depth\tmean_mapq\n";
		for (uint32_t r = 0; r < W.n_ref; ++r) {
			const urmapx_depth_summary &s = D.refs[r];
			const uint32_t len = W.ref_lens[r];
			rep.depth_covered += s.covered;
			rep.depth_bases += s.bases;
			char line[160];
			snprintf(line, sizeof line, "\t%u\t%llu\t%llu\t%.2f\t%.2f\t%.2f\n", len, (unsigned long long)s.reads, (unsigned long long)s.covered,
			         len ? 100.0 * (double)s.covered / len : 0.0, len ? (double)s.bases / len : 0.0, s.reads ? (double)s.mapq_sum / (double)s.reads : 0.0);
			table += W.ref_names[r];
			table += line;
		}
		return file_s;
	}
	// the statistics' file and the report's totals -> the file's seconds
	double write_stats(const Sorted &W) {
		const auto ts0 = now();
		const urmapx_stats_result &T = W.T;
		FileSink ssink;
		if (!ssink.open(opt.stats_out) || !ssink.write_at(T.text, T.text_bytes, 0, 1) || !ssink.finish(T.text_bytes))
			fail.raise(URMAPX_E_IO, std::string("Error writing ") + opt.stats_out);
		const double file_s = secs(ts0, now());
		rep.write_s += file_s;
		rep.stats_reads = T.reads; rep.stats_mapped = T.mapped; rep.stats_properly_paired = T.properly_paired;
		rep.stats_duplicated = T.duplicated; rep.stats_insert_median = T.insert_median;
		return file_s;
	}
	// the VCF file and the report's total -> the file's seconds
	double write_vcf(const Sorted &W) {
		const auto ts0 = now();
		const urmapx_pileup_result &V = W.V;
		FileSink vsink;
		if (!vsink.open(opt.vcf_out) || !vsink.write_at(V.text, V.text_bytes, 0, 1) || !vsink.finish(V.text_bytes))
			fail.raise(URMAPX_E_IO, std::string("Error writing ") + opt.vcf_out);
		const double file_s = secs(ts0, now());
		rep.write_s += file_s;
		rep.pileup_sites = V.sites; rep.pileup_records = V.records; rep.pileup_alt_alleles = V.alt_alleles;
		return file_s;
	}
	// the report's fields of the sort, the marking, the depth, the statistics and the pileup, and under URMAPX_VERBOSE their lines, which the scripts read:
	// scripts/bam_sort_bench.py, depth_bench.py, bam_sort_external_bench.py, markdup_bench.py, in this order
	void report_sorted(const Sorted &W, double sorted_s, double bam_s, double bed_s, double stats_file_s, double vcf_file_s) {
		const urmapx_bam_sort_result &S = W.S;
		const urmapx_markdup_stats &M = W.M;
		const urmapx_depth_result &D = W.D;
		const bool verbose = getenv("URMAPX_VERBOSE") != nullptr;
		if (verbose)  // the parts of sort_s
			fprintf(stderr, "bam_sort seconds: total %.4f scan %.4f alloc %.4f upload %.4f sort %.4f gather %.4f deflate %.4f copy %.4f index %.4f write %.4f; "
			                "records %llu bytes %llu passes %u slices %u\n",
			        sorted_s, S.scan_s, S.alloc_s, S.upload_s, S.sort_s, S.gather_s, S.deflate_s, S.copy_s, S.index_s, bam_s,
			        (unsigned long long)S.records, (unsigned long long)S.stream_bytes, S.sort_passes, S.slices);
		if (opt.depth_out) {
			rep.depth_s = D.alloc_s + D.count_s + D.scan_s + D.runs_s + D.format_s + D.copy_s + bed_s;
			if (verbose)
				fprintf(stderr, "depth seconds: total %.4f alloc %.4f count %.4f scan %.4f runs %.4f format %.4f copy %.4f write %.4f; runs %llu bytes %llu slices %u\n",
				        rep.depth_s, D.alloc_s, D.count_s, D.scan_s, D.runs_s, D.format_s, D.copy_s, bed_s, (unsigned long long)D.runs, (unsigned long long)D.text_bytes,
				        D.text_slices);
		}
		if (opt.stats_out) {
			const urmapx_stats_result &T = W.T;
			rep.stats_s = T.alloc_s + T.count_s + T.format_s + stats_file_s;
			if (verbose)
				fprintf(stderr, "stats seconds: total %.4f alloc %.4f count %.4f format %.4f write %.4f; records %llu bytes %llu\n", rep.stats_s, T.alloc_s, T.count_s,
				        T.format_s, stats_file_s, (unsigned long long)T.records, (unsigned long long)T.text_bytes);
		}
		if (opt.vcf_out) {
			const urmapx_pileup_result &V = W.V;
			rep.pileup_s = V.alloc_s + V.count_s + V.sites_s + V.format_s + V.copy_s + vcf_file_s;
			if (verbose)
				fprintf(stderr, "pileup seconds: total %.4f alloc %.4f count %.4f sites %.4f format %.4f copy %.4f write %.4f; records %llu sites %llu alleles %llu bytes %llu\n",
				        rep.pileup_s, V.alloc_s, V.count_s, V.sites_s, V.format_s, V.copy_s, vcf_file_s, (unsigned long long)V.records, (unsigned long long)V.sites,
				        (unsigned long long)V.alt_alleles, (unsigned long long)V.text_bytes);
		}
		rep.sort_partitions = S.external ? S.partitions : 0;
		if (S.external && verbose)
			fprintf(stderr, "bam_sort external: partitions %u chunks %llu passes %u stage %.4f\n", S.partitions, (unsigned long long)S.stage_chunks, S.partitions + 1u, S.stage_s);
		if (opt.markdup) {
			rep.pairs_examined = M.pairs_examined; rep.pairs_duplicate = M.pairs_duplicate;
			rep.fragments_examined = M.fragments_examined; rep.fragments_duplicate = M.fragments_duplicate;
			rep.markdup_s = M.markdup_s;
			if (verbose)
				fprintf(stderr, "markdup seconds: %.4f; pairs %llu duplicate %llu fragments %llu duplicate %llu\n", M.markdup_s, (unsigned long long)M.pairs_examined,
				        (unsigned long long)M.pairs_duplicate, (unsigned long long)M.fragments_examined, (unsigned long long)M.fragments_duplicate);
		}
	}
	int finish(urmapx_map_report *report, std::string &msg) {
		if (sort && !fail.set.load()) write_sorted();
		if (bgzf && !fail.set.load()) {  // htslib's empty member: the file is complete
			std::string eof;
			(void)bgzf_members(eof, 1);
			if (!sink.write_at(eof.data(), eof.size(), rep.sam_file_bytes, 1)) cannot_write_sam();
			rep.sam_file_bytes += eof.size();
		}
		if (have_sam && !sink.finish(rep.sam_file_bytes)) cannot_write_sam();
		if (sort && fail.set.load()) {  // a failed sorted run leaves neither file
			remove(samout);
			remove((std::string(samout) + ".bai").c_str());
			if (opt.depth_out) remove(opt.depth_out);
			if (opt.stats_out) remove(opt.stats_out);
			if (opt.vcf_out) remove(opt.vcf_out);
		}
		ftab.reset();  // (inside the run's clock; the lanes are let go outside it)
		const auto t2 = now();
		range.t_begin = std::chrono::duration<double>(t1.time_since_epoch()).count();
		range.t_end = std::chrono::duration<double>(t2.time_since_epoch()).count();
		trace.dump();
		run_ok = !fail.set.load();
		close();
		if (report) {
			rep.seconds = secs(t1, t2);
			memcpy(&rep.shard_scan_s, &report->shard_scan_s, sizeof rep.shard_scan_s);  // the sharded caller's field (alloc_* are filled by urmapx_map_files afterwards)
			*report = rep;
		}
		if (fail.set.load()) return failed(fail.code, msg, fail.msg);
		return rep.unsupported ? URMAPX_E_UNSUPPORTED : URMAPX_OK;
	}
};

// ---- text phase: reads from plain files, FASTQ bytes -> device -> SAM bytes ----
// Threads: reader (stream or plain file), a lane per context, writer.  Chunk b: free_jobs -> reader -> parsed[b mod lanes] -> lane -> mapped[b mod lanes] -> writer.
struct TextPhase {
	using TextChannel = Channel<std::unique_ptr<TextJob>>;
	Run &R;
	std::vector<std::unique_ptr<TextChannel>> parsed, mapped;
	const int n_jobs = 3 * R.n_lanes + 2;  // per lane: one waiting for it, one being mapped, one whose text is crossing PCIe; reader, writer
	TextChannel free_jobs{(size_t)n_jobs};
	int fq = -1, fq2 = -1;
	uint64_t fsize = 0, fsize2 = 0;
	SeqSource src1, src2;
	bool streamed = false;
	size_t chunk_bytes = 0;
	const int read_threads = std::max(1, R.host_threads / 2);
	// write() calls on one file take turns (inode lock): more threads only add hand-overs
	const int write_threads = R.sink.writer_threads(R.host_threads);
	std::atomic<bool> stop{false};  // set by the writer: a chunk was handed back
	// No page-locked memory for a chunk (memlock limit, little host memory), or none on the device for the text kernels:
	// the text phase ends there and the host reader / formatter, which need neither, continue from that chunk.
	std::atomic<bool> nomem{false};
	// -- the reader thread's; read by leaves_work() after the joins --
	uint64_t off = R.range.on ? R.range.lo[0] : 0, off2 = R.range.on ? R.range.lo[1] : 0;  // first byte of each file the reader did not hand to a lane
	bool stream_done = false;  // streamed input: the reader handed every byte of the input(s) to a lane
	// streamed input: bytes read from each source and not handed to a lane yet (behind the last cut; a whole buffer the
	// reader gave up on).  Pipes: they go to the host reader in front of the rest of the pipe, behind pipe_back.
	std::vector<char> carry, carry2;
	double bytes2_per_byte1 = 1.0;
	std::vector<size_t> per;
	// -- the writer thread's; read by leaves_work() after the joins --
	bool handed_back = false;
	uint64_t resume_off = 0, resume_off2 = 0, lines_done = R.range.on ? R.range.lines_before : 0;  // lines_done: per file
	std::vector<char> pipe_back, pipe_back2;
	bool going() const { return !stop.load() && !R.fail.set.load() && !nomem.load(); }
	// false: this input does not take the text road (no SAM wanted, a tab file without pairs, URMAPX_HOST_TEXT, a file that cannot be opened)
	bool open_input() {
		// -tabbedout (pairs only): the SAM text is made on the device all the same; the lines of the tab file are formatted by
		// host threads from the chunk's results and pair records (urmapx_text_fetch_pairs), with the labels read in place
		if (!R.have_sam || (R.ftab && !R.paired) || getenv("URMAPX_HOST_TEXT")) return false;
		// .gz input: the same phase with the chunks cut out of the inflated stream (SeqSource).  A pipe (FIFO, standard input)
		// is streamed the same way; it has no way back to a chunk the device parser hands back, so the bytes of that chunk
		// and of everything read behind it are kept and given to the host reader in front of the rest of the pipe.
		auto open_src = [](SeqSource &src, FastqReader &r, const char *path) {
			if (r.is_pipe()) return src.open_pipe(r.fd());
			return strcmp(path, "-") != 0 && src.open(path, is_gz_name(path));
		};
		if (is_gz_name(R.fastq1) || (R.paired && is_gz_name(R.fastq2)) || R.rd.is_pipe() || (R.paired && R.rd2.is_pipe())) {
			streamed = open_src(src1, R.rd, R.fastq1) && (!R.paired || open_src(src2, R.rd2, R.fastq2));
			src1.set_gz_threads(R.host_threads);  // a plain gzip stream: the inflater is what the run waits for
			src2.set_gz_threads(R.host_threads);
			return streamed;
		}
		fq = open_plain(R.fastq1, fsize);
		if (fq >= 0 && R.paired) {
			fq2 = open_plain(R.fastq2, fsize2);
			if (fq2 < 0) { close(fq); fq = -1; }
		}
		if (fq >= 0 && R.range.on) { fsize = R.range.hi[0]; fsize2 = R.range.hi[1]; }  // a shard: its part of the file(s) is the file
		return fq >= 0;
	}
	void choose_chunk_bytes() {
		const bool paired = R.paired;
		const uint32_t batch = R.batch;
		chunk_bytes = (size_t)std::min(330.0 * (double)(paired ? std::max(1u, batch / 2) : batch), 536870912.0);  // streamed: a 150-base record
		if (streamed && !R.opt.batch && src1.is_gz()) {
			// no -batch given: larger chunks for a large file, as for plain input below (FASTQ text is 4-5 times its gzip size)
			const double est = 4.0 * (double)src1.compressed_size() / 330.0 * (paired ? 2.0 : 1.0);
			const double reads = std::min(524288.0, std::max((double)batch, est / (4.0 * (double)R.n_lanes)));
			chunk_bytes = (size_t)std::min(330.0 * (paired ? std::max(1.0, reads / 2) : reads), 536870912.0);
		}
		if (streamed) return;
		// `batch` reads (pairs: batch / 2 of each file) at the record size the head of the file shows
		std::vector<char> head(1u << 16);
		const ssize_t k = pread(fq, head.data(), head.size(), 0);
		size_t nl = 0, last = 0;
		for (ssize_t i = 0; i < k; ++i)
			if (head[(size_t)i] == '\n' && (++nl & 3) == 0) last = (size_t)i + 1;
		const double rec = nl >= 4 ? (double)last / (double)(nl / 4) : 512.0;
		double reads_per_chunk = (double)batch;
		if (!R.opt.batch) {
			// no -batch given: a chunk pays 3-4 ms of fixed cost on the device (launch tails, the second pass's empty launches) --
			// two thirds of a 262 144-read chunk's mapping time at 46 M reads/s -- so a large file is cut into larger chunks, up to
			// 524 288 reads, as long as every lane still gets four of them (the lanes overlap each other's copies).  Measured on
			// 10 M reads (profiles/r5/e2e_by_chunk.txt): 262 144 -> 29.2 M reads/s with the SAM text dropped, 524 288 -> 31.2 M;
			// 1 M-read chunks need 0.7 GB of page-locked memory each, six of them outgrow the pool and the run stalls in
			// hipHostMalloc / hipHostFree (6.5 M reads/s)
			const double est = (double)(fsize - (R.range.on ? R.range.lo[0] : 0)) / rec * (paired ? 2.0 : 1.0);
			reads_per_chunk = std::min(524288.0, std::max((double)batch, est / (4.0 * (double)R.n_lanes)));
			if (const char *e = getenv("URMAPX_TEST_CHUNK_READS")) reads_per_chunk = std::max(4.0, atof(e));  // test aid: the library's own choice, small (the ramp below on a small file)
		}
		chunk_bytes = (size_t)std::min(std::max(rec * (paired ? std::max(1.0, reads_per_chunk / 2) : reads_per_chunk), 4096.0), 536870912.0);
	}
	void run() {
		choose_chunk_bytes();
		for (int l = 0; l < R.n_lanes; ++l) {
			parsed.emplace_back(new TextChannel(1));
			mapped.emplace_back(new TextChannel(1));
		}
		for (int k = 0; k < n_jobs; ++k) free_jobs.push(std::make_unique<TextJob>());
		R.rep.write_threads = write_threads;
		R.rep.text_on_device = 1;
		std::thread treader([this] { reader(); });
		std::thread twriter([this] { writer(); });
		std::vector<std::thread> tlanes;
		for (int l = 0; l < R.n_lanes; ++l) tlanes.emplace_back([this, l] { lane(l); });
		for (auto &t : tlanes) t.join();
		treader.join();
		twriter.join();
		const auto tf = now();
		std::unique_ptr<TextJob> j;
		while (free_jobs.try_pop(j)) j.reset();
		R.trace.add("unpin", -1, 0, tf);
		if (fq >= 0) close(fq);
		if (fq2 >= 0) close(fq2);
	}
	// After the joins: does the host phase have work?  Then the host readers stand where the text phase stopped.
	bool leaves_work() {
		if (!handed_back) { resume_off = off; resume_off2 = off2; }
		if (R.fail.set.load()) return false;
		if (streamed ? !(handed_back || !stream_done) : !(resume_off < fsize || (R.paired && resume_off2 < fsize2))) return false;
		// a seekable source continues at its (uncompressed) offset; a pipe with the bytes taken from it and not mapped
		auto resume = [&](FastqReader &r, SeqSource &src, uint64_t at, std::vector<char> &back, std::vector<char> &rest) {
			if (!streamed || !src.is_pipe()) return r.resume_at(at, lines_done);  // (a shard's reader: positioned again, same rules)
			back.insert(back.end(), rest.begin(), rest.end());
			return r.resume_with_prefix(std::move(back), lines_done);
		};
		if (!resume(R.rd, src1, resume_off, pipe_back, carry) || (R.paired && !resume(R.rd2, src2, resume_off2, pipe_back2, carry2)))
			R.fail.raise(URMAPX_E_IO, std::string("Cannot continue reading ") + R.fastq1);
		return !R.fail.set.load();
	}
	void to_lane(std::unique_ptr<TextJob> &j, size_t b, const char *what, Clock::time_point since) {
		R.rep.parse_s += secs(since, now());
		R.trace.add(what, -1, b, since);
		off += j->nbytes; off2 += j->nbytes2;
		parsed[b % (size_t)R.n_lanes]->push(std::move(j));
	}
	void reader() {
		const bool pinned = R.one_node && pin_to(R.places[0]);  // the page-locked chunk buffers are first touched here
		Unpin unpin{pinned, R.caller_mask, read_threads};
		omp_team(read_threads);
		if (streamed) read_stream();
		else read_plain();
		for (auto &c : parsed) c->close();
	}
	// Chunks are cut out of the inflated stream: fill the job's buffer (what the last cut left over first), cut it at its last record
	// start, keep the rest for the next chunk.  Offsets are those of the uncompressed text: that is where the host reader (gzseek) takes
	// over if a chunk is handed back.
	void read_stream() {
		bool eof1 = false, eof2 = false;
		for (size_t b = 0; going(); ++b) {
			if (eof1 && carry.empty()) { stream_done = !R.paired || (eof2 && carry2.empty()); break; }
			std::unique_ptr<TextJob> j;
			if (!free_jobs.pop(j)) break;
			if (stop.load()) { free_jobs.push(std::move(j)); break; }
			const auto tp0 = now();
			(void)hipSetDevice(R.phys(0));
			size_t area1 = chunk_bytes + chunk_bytes / 8 + carry.size() + (1u << 20);  // room for this file's chunk
			const size_t area2 = R.paired ? (size_t)((double)area1 * bytes2_per_byte1 * 1.25) + carry2.size() + (4u << 20) : 0;
			if (!TextJob::grow(j->in, j->in_cap, area1 + 4096 + area2)) { nomem.store(true); break; }
			size_t n = carry.size(), cut = 0;
			if (n) memcpy(j->in, carry.data(), n);
			carry.clear();
			size_t target = std::max(chunk_bytes, n + 1);
			for (;;) {
				while (n < target && !eof1) {
					const size_t k = src1.read(j->in + n, std::min(area1, target + (64u << 10)) - n, read_threads);
					if (k == 0) eof1 = true;
					n += k;
					// a gzip stream's reader hands out whole rounds written straight into this buffer and returns short when the next round
					// would not fit (pgzip.cpp): a chunk that is three quarters full is a chunk -- asking for the rest would cost a copy of a whole round
					if (src1.returns_whole_rounds() && n >= target - target / 4) break;
				}
				if (src1.failed()) break;
				cut = eof1 ? n : last_record_start(j->in, n);
				if (cut || eof1) break;
				target *= 2;  // less than one record start in the buffer: records of a size beyond reason, or not FASTQ
				if (target > (1u << 30)) break;
				if (target + (64u << 10) > area1) {
					area1 = target + target / 8 + (1u << 20);
					if (!regrow(*j, area1 + 4096 + area2, n)) { nomem.store(true); break; }
				}
			}
			if (R.fail.set.load() || nomem.load()) { carry.assign(j->in, j->in + n); break; }
			if (src1.failed()) { R.fail.raise(URMAPX_E_IO, std::string(src1.is_pipe() ? "Error reading " : "Error reading gzip file ") + R.fastq1); break; }
			if (cut == 0) { carry.assign(j->in, j->in + n); free_jobs.push(std::move(j)); break; }  // the host reader says what is wrong with it
			carry.assign(j->in + cut, j->in + n);
			j->nbytes = cut; j->file_off = off; j->nbytes2 = 0; j->file_off2 = off2; j->in2 = nullptr;
			if (R.paired && !cut_mate_stream(*j, cut, area1, area2, eof1 && carry.empty(), eof2)) { free_jobs.push(std::move(j)); break; }
			to_lane(j, b, "inflate", tp0);
		}
	}
	// The mate stream's chunk: as many lines as j's first `cut` bytes hold; every byte is looked at once (`scanned`).  false: the chunk stays
	// with the reader, both files' bytes are back in the carries.
	bool cut_mate_stream(TextJob &j, size_t cut, size_t area1, size_t area2, bool last, bool &eof2) {
		const size_t lines = count_lines(j.in, cut, read_threads, per);
		MateChunk m{j, cut, (area1 + 4095) & ~(size_t)4095};
		if (carry2.size() > area2) {
			area2 = carry2.size() + carry2.size() / 4 + (4u << 20);
			if (!m.grow(area2)) { nomem.store(true); m.give_up = true; }
		}
		if (!m.give_up) {
			if (!carry2.empty()) memcpy(m.dst(), carry2.data(), carry2.size());
			m.have = carry2.size();
			carry2.clear();
		}
		size_t seen = 0, scanned = 0;
		while (!m.found && !m.give_up) {
			// newlines of dst[scanned, have): the chunk ends behind line number `lines`
			const char *c = m.dst() + scanned, *e = m.dst() + m.have;
			while (c < e && (last || seen < lines)) {
				const char *nl = (const char *)memchr(c, '\n', (size_t)(e - c));
				if (!nl) break;
				++seen;
				c = nl + 1;
				if (!last && seen == lines) m.end_at((size_t)(c - m.dst()));
			}
			scanned = (size_t)(c - m.dst());
			if (m.found) break;
			if (eof2) { if (last) m.end_at(m.have); else m.give_up = true; break; }  // the mate file ends first: the host reader words that
			if (m.have == area2) {
				if (area2 > 8 * area1 + (64u << 20)) { m.give_up = true; break; }
				if (!m.grow(2 * area2)) { nomem.store(true); m.give_up = true; break; }
				area2 *= 2;
			}
			const size_t expect = (size_t)((double)cut * bytes2_per_byte1);
			const size_t want = std::min(area2 - m.have, std::max<size_t>(1u << 20, expect + (64u << 10) - std::min(m.have, expect)));
			const size_t k = src2.read(m.dst() + m.have, want, read_threads);
			if (k == 0) eof2 = true;
			m.have += k;
			if (src2.failed()) { R.fail.raise(URMAPX_E_IO, std::string(src2.is_pipe() ? "Error reading " : "Error reading gzip file ") + R.fastq2); m.give_up = true; }
		}
		if (m.give_up || R.fail.set.load() || nomem.load()) {
			carry.insert(carry.begin(), j.in, j.in + cut);
			carry2.insert(carry2.begin(), m.dst(), m.dst() + m.have);
			return false;
		}
		carry2.assign(m.dst() + m.n2, m.dst() + m.have);
		m.hand_to_job(bytes2_per_byte1);
		return true;
	}
	void read_plain() {
		// Round 6: the library's own chunk size (no -batch given) is ramped.  The first chunk of a lane is a quarter of the size, its second
		// a half: the lanes start after 40 MB have been read instead of 165 MB, and the second lane a quarter-chunk later instead of a whole
		// one.  The last round of chunks is cut in halves again and again (down to an eighth), so that the run does not end with one lane
		// mapping a whole chunk while the others have nothing left (10 M reads: 19 chunks of 13 ms, of which the first and the last ran
		// beside an idle lane).  URMAPX_NO_CHUNK_RAMP=1: every chunk the same size (measurement).
		const bool ramp = !R.opt.batch && !getenv("URMAPX_NO_CHUNK_RAMP");
		const size_t n_lanes = (size_t)R.n_lanes;
		for (size_t b = 0; off < fsize && going(); ++b) {
			uint64_t end = fsize;
			size_t this_chunk = chunk_bytes;
			if (ramp) {
				if (b < n_lanes) this_chunk = chunk_bytes / 4;
				else if (b < 2 * n_lanes) this_chunk = chunk_bytes / 2;
				const uint64_t left = fsize - off;
				if (left <= (uint64_t)n_lanes * chunk_bytes) this_chunk = (size_t)std::min<uint64_t>(this_chunk, std::max<uint64_t>(left / (2 * (uint64_t)n_lanes), chunk_bytes / 8));
				this_chunk = std::max<size_t>(this_chunk, 1024);
			}
			if (off + this_chunk < fsize) {
				end = find_record_start(fq, off + this_chunk, fsize);
				if (end == 0) break;  // no record start in sight: the host reader takes it from here
			}
			std::unique_ptr<TextJob> j;
			if (!free_jobs.pop(j)) break;
			if (stop.load()) break;
			const size_t n = (size_t)(end - off);
			const auto tp0 = now();
			(void)hipSetDevice(R.phys(0));
			const size_t n_pad = (n + 4095) & ~(size_t)4095;  // the mate file's chunk starts here
			size_t want = n + n / 16 + 4096;
			if (R.paired) want = n_pad + (size_t)((double)n * bytes2_per_byte1 * 1.25) + (4u << 20);
			if (!TextJob::grow(j->in, j->in_cap, want)) { nomem.store(true); break; }
			if (!read_range(fq, j->in, off, n, read_threads)) { R.fail.raise(URMAPX_E_IO, std::string("Error reading ") + R.fastq1); break; }
			j->nbytes = n; j->file_off = off; j->nbytes2 = 0; j->file_off2 = off2; j->in2 = nullptr;
			if (R.paired && !cut_mate_plain(*j, n, n_pad, end == fsize)) { free_jobs.push(std::move(j)); break; }
			to_lane(j, b, "read", tp0);
		}
	}
	// The mate file's chunk: as many lines as j's first n bytes hold; what has been read is counted again by all reader threads after
	// every piece.  false: the chunk stays with the reader, the host reader continues at its first byte.
	bool cut_mate_plain(TextJob &j, size_t n, size_t n_pad, bool last) {
		const size_t lines = count_lines(j.in, n, read_threads, per);
		MateChunk m{j, n, n_pad};
		auto room = [&] { return j.in_cap - n_pad; };
		const uint64_t left2 = fsize2 - off2;
		auto read_to = [&](size_t upto) {
			const bool ok = read_range(fq2, m.dst() + m.have, off2 + m.have, upto - m.have, read_threads);
			if (!ok) { R.fail.raise(URMAPX_E_IO, std::string("Error reading ") + R.fastq2); m.give_up = true; }
			m.have = upto;
			return ok;
		};
		if (last) {  // last chunk: whatever the mate file still holds (the device parser says if it is not the same count)
			if (left2 > room() && (left2 > 8ull * n + (64u << 20) || !m.grow((size_t)left2 + (4u << 20)))) m.give_up = true;
			else if (read_to((size_t)left2)) m.end_at(m.have);
		}
		while (!m.found && !m.give_up) {
			size_t upto = m.have ? m.have + m.have / 4 + (1u << 20) : (size_t)((double)n * bytes2_per_byte1) + (1u << 16);
			upto = (size_t)std::min<uint64_t>(std::min<uint64_t>(upto, room()), left2);
			if (upto <= m.have) {
				if (m.have < left2 && room() < 8 * n + (64u << 20) && m.grow(2 * room() + (4u << 20))) continue;  // out of room, not out of file
				m.give_up = true;  // out of file with too few lines (the host reader words that), or a chunk beyond reason
				break;
			}
			if (!read_to(upto)) break;
			count_lines(m.dst(), m.have, read_threads, per);
			if (const size_t n2 = nth_line_end(m.dst(), m.have, per, lines)) m.end_at(n2);
			else if (m.have == left2) m.give_up = true;  // the mate file ends first: the host reader words that
		}
		if (m.give_up || R.fail.set.load() || nomem.load()) return false;
		m.hand_to_job(bytes2_per_byte1);
		return true;
	}
	void format_tab(TextJob &j) {
		const uint32_t np = j.rep.records / 2;
		const int TT = std::max(1, R.host_threads / R.n_lanes);
		std::vector<std::string> parts((size_t)TT);
#pragma omp parallel for schedule(static, 1) num_threads(TT)
		for (int t = 0; t < TT; ++t) {
			std::string &o = parts[(size_t)t];
			const uint32_t lo = (uint32_t)part(np, t, TT), hi = (uint32_t)part(np, t + 1, TT);
			o.reserve((size_t)(hi - lo) * 72);
			for (uint32_t u = lo; u < hi; ++u) {
				const uint32_t *e = j.tab_ends.data() + (size_t)4 * u;
				const uint32_t s0 = (u ? e[-1] + 1u : 0u) + 1u;  // behind the '@'
				append_tab_pe(o, R.I, &j.tab_res[(size_t)2 * u], &j.tab_res[(size_t)2 * u + 1], &j.tab_info[u], j.in + s0, e[0] - s0,
				              e[1] - e[0] - 1u, j.tab_lens2[u], R.have_sam ? 1 : 0);
			}
		}
		for (const std::string &o : parts) j.tab += o;
	}
	void lane(int l) {
		omp_workers_sleep_when_idle();
		const bool pinned = pin_to(R.places[(size_t)(l % R.gpus)]);
		Unpin unpin{pinned, R.caller_mask, std::max(1, R.host_threads / R.n_lanes)};
		(void)hipSetDevice(R.phys(l % R.gpus));
		urmapx_text *T = R.texts[(size_t)l];
		const auto tc = now();
		const int trc = T ? URMAPX_OK : urmapx_text_create(R.ctxs[(size_t)l], &T);
		R.texts[(size_t)l] = T;  // released with the lane's context (kept for the next call, or destroyed)
		R.trace.add("create", l, 0, tc);
		size_t nj = 0;
		double sam_per_fastq = 1.12;
		if (trc == URMAPX_E_NOMEM) nomem.store(true);  // T stays null: this lane's chunks go back unmapped
		else if (trc) R.fail.raise(trc, std::string("urmapx_text_create: ") + urmapx_strerror(trc));
		if (T) {
			const int brc = urmapx_text_set_bgzf(T, R.bgzf ? 1 : 0);  // (a lane from the pool keeps what its last run set)
			int brc2 = 0;
			if (brc == URMAPX_E_NOMEM) { nomem.store(true); T = nullptr; }
			else if (brc) R.fail.raise(brc, std::string("urmapx_text_set_bgzf: ") + urmapx_strerror(brc));
			else if ((brc2 = urmapx_text_set_bam(T, R.bam ? 1 : 0))) R.fail.raise(brc2, std::string("urmapx_text_set_bam: ") + urmapx_strerror(brc2));
			else if ((brc2 = urmapx_text_set_tags(T, R.tags, R.rg_line ? R.rg_id.c_str() : nullptr))) R.fail.raise(brc2, std::string("urmapx_text_set_tags: ") + urmapx_strerror(brc2));
		}
		// The copy back is a stage of its own (urmapx_text_set_deferred): chunk i's text crosses PCIe while the lane's stream takes
		// chunk i + 1 in and maps it; the lane waits for chunk i's copy when chunk i + 1 has been enqueued to its end.
		// URMAPX_NO_DEFERRED_COPY=1 (measurement): every chunk is waited for before the next is taken.
		const bool defer = T && !getenv("URMAPX_NO_DEFERRED_COPY") && urmapx_text_set_deferred(T, 1) == URMAPX_OK;
		auto ok_so_far = [](const TextJob &q) { return !q.rc && (q.rep.reason == 0 || q.rep.reason == URMAPX_TEXT_DEFERRED); };
		auto hand_on = [&](std::unique_ptr<TextJob> &q) {
			if (!q->rc && q->rep.reason == URMAPX_TEXT_DEFERRED) {
				const auto tw0 = now();
					q->rc = urmapx_text_wait(T, &q->rep);
				R.trace.add("wait", l, 0, tw0);
				R.add_lane_time(&Rep::gpu_s, tw0);
			}
			mapped[(size_t)l]->push(std::move(q));
		};
		std::unique_ptr<TextJob> j, prev;
		while (parsed[(size_t)l]->pop(j)) {
			memset(&j->rep, 0, sizeof j->rep);
			j->rc = 0;
			if (T && !R.fail.set.load() && !stop.load()) {
				const auto tg0 = now();
					// the SAM buffer is sized from the previous chunk's text (150-base reads: 1.09 x their FASTQ text); a chunk
				// that needs more says so and its text is fetched into a larger one
				const size_t fq_bytes = j->nbytes + j->nbytes2;
				if (!TextJob::grow(j->out, j->out_cap, (size_t)((double)fq_bytes * sam_per_fastq * 1.04) + (1u << 20))) j->rc = URMAPX_E_NOMEM;
				if (!j->rc)
					j->rc = R.paired ? urmapx_text_map_pe(T, j->in, j->nbytes, j->in2, j->nbytes2, R.minq, j->out, j->out_cap, &j->rep)
					                 : urmapx_text_map_se(T, j->in, j->nbytes, R.minq, j->out, j->out_cap, &j->rep);
				if (!j->rc && j->rep.reason == URMAPX_TEXT_SAM_CAP) {
					if (!TextJob::grow(j->out, j->out_cap, (size_t)j->rep.sam_bytes + j->rep.sam_bytes / 16 + (1u << 20))) j->rc = URMAPX_E_NOMEM;
					else j->rc = urmapx_text_fetch_sam(T, j->out, j->out_cap, &j->rep);
				}
				// (under bgzf the buffer takes the worst case of the text, a 2100th more than the text itself)
				if (ok_so_far(*j) && fq_bytes && j->rep.records) sam_per_fastq = (double)j->rep.sam_text_bytes / (double)fq_bytes * (R.bgzf ? 1.001 : 1.0);
				j->tab.clear();
				if (ok_so_far(*j) && R.ftab && j->rep.records) {
					const uint32_t np = j->rep.records / 2;
					j->tab_res.resize((size_t)2 * np); j->tab_info.resize(np); j->tab_ends.resize((size_t)4 * np); j->tab_lens2.resize(np);
					j->rc = urmapx_text_fetch_pairs(T, np, j->tab_res.data(), j->tab_info.data(), j->tab_ends.data(), j->tab_lens2.data());
					if (!j->rc) {
						const auto tf0 = now();
						format_tab(*j);
						R.add_lane_time(&Rep::format_s, tf0);
					}
				}
				R.trace.add("gpu", l, (size_t)l + nj * (size_t)R.n_lanes, tg0);
				R.add_lane_time(&Rep::gpu_s, tg0);
			} else
				j->rep.reason = 0xFFFFu;  // not mapped: the phase is ending
			if (prev) hand_on(prev);
			if (defer) prev = std::move(j);
			else mapped[(size_t)l]->push(std::move(j));
			++nj;
		}
		if (prev) hand_on(prev);
		mapped[(size_t)l]->close();
	}
	// Chunks come back in input order (the lanes in turn).  The first one the device parser did not take ends the phase: nothing from it on
	// is written; a pipe's bytes are kept for the host reader.
	void writer() {
		const bool pinned = R.one_node && pin_to(R.places[0]);
		Unpin unpin{pinned, R.caller_mask, R.host_threads};
		omp_team(R.host_threads);
		std::unique_ptr<TextJob> j;
		for (size_t b = 0; mapped[b % (size_t)R.n_lanes]->pop(j); ++b) {
			if (!handed_back && !R.fail.set.load()) {
				if (j->rc == URMAPX_E_NOMEM) { j->rc = 0; j->rep.reason = 0xFFFEu; nomem.store(true); }
				if (j->rc) R.fail.raise(j->rc, std::string(R.paired ? "urmapx_text_map_pe: " : "urmapx_text_map_se: ") + urmapx_strerror(j->rc));
				else if (j->rep.reason) { handed_back = true; stop.store(true); resume_off = j->file_off; resume_off2 = j->file_off2; }
			}
			if (handed_back && streamed) {  // pipes: this chunk's bytes and those of every chunk behind it, in order
				if (src1.is_pipe()) pipe_back.insert(pipe_back.end(), j->in, j->in + j->nbytes);
				if (R.paired && src2.is_pipe() && j->in2) pipe_back2.insert(pipe_back2.end(), j->in2, j->in2 + j->nbytes2);
			}
			if (!handed_back && !R.fail.set.load()) {
				const auto tw0 = now();
	#ifdef URX_FAULT_OFF32  // fault injection for the suite's own check (profiles/r6/fault_off32.txt): the writer's file offset cut to 32 bits
				const uint64_t at = (uint32_t)R.rep.sam_file_bytes;
#else
				const uint64_t at = R.rep.sam_file_bytes;
#endif
				if (!R.sink.write_at(j->out, (size_t)j->rep.sam_bytes, at, write_threads)) R.cannot_write_sam();
				R.rep.sam_file_bytes += j->rep.sam_bytes;
				if (R.ftab && !j->tab.empty() && fwrite(j->tab.data(), 1, j->tab.size(), R.ftab.get()) != j->tab.size())
					R.fail.raise(URMAPX_E_IO, std::string("Error writing ") + R.tabout);
				R.rep.write_s += secs(tw0, now());
				R.trace.add("write", -1, b, tw0);
				urmapx_map_report &r = R.rep;
				const urmapx_text_report &c = j->rep;
				r.reads += c.records; r.mapped_q += c.mapped_q; r.mapped_lowq += c.mapped_lowq; r.unmapped += c.unmapped; r.unsupported += c.unsupported;
				r.sam_text_bytes += c.sam_text_bytes;
				r.dev_h2d_s += c.ms_h2d * 1e-3; r.dev_parse_s += c.ms_parse * 1e-3; r.dev_map_s += c.ms_map * 1e-3; r.dev_format_s += c.ms_format * 1e-3;
				r.dev_d2h_s += c.ms_d2h * 1e-3; r.dev_map_search_s += c.ms_map_search * 1e-3; r.dev_map_dp_s += c.ms_map_dp * 1e-3;
				r.map_enqueue_s += c.ms_map_enqueue * 1e-3;
				lines_done += (R.paired ? 2ull : 4ull) * j->rep.records;
				R.rep.input_bytes += j->nbytes + j->nbytes2;
			}
			free_jobs.push(std::move(j));
		}
	}
};

// ---- host phase: FASTQ parsed, SAM formatted and written by host threads; the lanes map arrays of reads ----
// Batch b travels through parsed[b mod lanes] -> lane thread -> mapped[b mod lanes]; the formatter visits the lanes in the same
// round-robin order, so batches come back in input order without a reorder buffer
struct HostPhase {
	using JobChannel = Channel<std::unique_ptr<Job>>;
	// SAM text of a batch is formatted by all host threads, each on a contiguous range of reads (pairs); the pieces go to
	// the flusher thread, which writes them at their file offsets (input order) while the next batch is being formatted.
	struct Text { std::vector<std::string> outs; std::vector<uint64_t> at; };
	struct Cnt { unsigned long long accept = 0, reject = 0, nohit = 0, unsupported = 0, text = 0; };  // of one formatting thread's share of a batch
	Run &R;
	std::vector<std::unique_ptr<JobChannel>> parsed, mapped;
	JobChannel recycled{(size_t)(8 + 6 * R.n_lanes)};  // finished jobs go back to the reader: their arrays are reused
	// -map2: the second file is parsed by its own thread while the reader parses the first
	struct Side { FastqBatch b; std::string e; bool more = false; } side2;  // the mate reader's between go2 and done2, else the reader's
	Channel<int> go2{1}, done2{1};
	Channel<std::unique_ptr<Text>> to_flush{2}, text_pool{4};
	void run() {
		for (int l = 0; l < R.n_lanes; ++l) {
			parsed.emplace_back(new JobChannel(2));
			mapped.emplace_back(new JobChannel(1));
		}
		std::thread treader2;
		if (R.paired) treader2 = std::thread([this] { mate_reader(); });
		std::thread treader([this] { reader(); });
		std::thread tflusher([this] { flusher(); });
		std::thread tformatter([this] { formatter(); });
		std::vector<std::thread> tlanes;
		for (int l = 0; l < R.n_lanes; ++l) tlanes.emplace_back([this, l] { lane(l); });
		for (auto &t : tlanes) t.join();
		treader.join();
		if (treader2.joinable()) treader2.join();
		tformatter.join();
		tflusher.join();
		// page-locked arrays are released before their contexts go
		std::unique_ptr<Job> j;
		while (recycled.try_pop(j)) j.reset();
	}
	void mate_reader() {
		omp_team(std::max(1, R.host_threads / 2));  // a new thread starts from the default team size, not main's
		int x;
		while (go2.pop(x)) {
			side2.b.clear();
			side2.e.clear();
			side2.more = R.rd2.next_batch(side2.b, R.batch / 2, side2.e);
			done2.push(1);
		}
	}
	void reader() {
		const int own_team = R.paired ? std::max(1, R.host_threads - R.host_threads / 2) : R.host_threads;
		omp_team(own_team);
		FastqBatch a;
		for (size_t b = 0; !R.fail.set.load(); ++b) {
			std::unique_ptr<Job> j;
			if (!recycled.try_pop(j)) j = std::make_unique<Job>();
			j->reads.clear();
			std::string e;
			bool more;
			const auto tp0 = now();
			if (!R.paired)
				more = R.rd.next_batch(j->reads, R.batch, e);
			else {  // mates interleaved: reads 2i, 2i+1 (map2.cpp:27-32 reads one record from each file under one lock)
				go2.push(1);
				a.clear();
				more = R.rd.next_batch(a, R.batch / 2, e);
				int x;
				done2.pop(x);
				const FastqBatch &bb = side2.b;
				if (e.empty()) e = side2.e;
				if (e.empty() && (more != side2.more || a.size() != bb.size())) e = std::string("Premature end of file in FASTQ") + (a.size() > bb.size() ? "2" : "1");
				if (e.empty()) {
					omp_team(R.host_threads);
					interleave_batches(a, bb, j->reads);
					omp_team(own_team);
				}
			}
			R.rep.parse_s += secs(tp0, now());
			if (!e.empty()) { R.fail.raise(URMAPX_E_FORMAT, e); break; }
			if (!more) break;
			parsed[b % (size_t)R.n_lanes]->push(std::move(j));
		}
		for (auto &c : parsed) c->close();
		go2.close();
	}
	void lane(int l) {
		urmapx_ctx *C = R.ctxs[(size_t)l];
		omp_workers_sleep_when_idle();
		const bool pinned = pin_to(R.places[(size_t)(l % R.gpus)]);
		Unpin unpin{pinned, R.caller_mask, 1};
		(void)hipSetDevice(R.phys(l % R.gpus));
		std::unique_ptr<Job> j;
		while (parsed[(size_t)l]->pop(j)) {
			const uint32_t n = j->reads.size();
			if (!R.fail.set.load()) {
				j->results.resize(n);
				j->ops.resize((size_t)n * URMAPX_MAX_PATH_OPS);
				// page-lock what crosses PCIe (the arrays are recycled, so this happens once per job object and size)
				if (!getenv("URMAPX_NO_PIN")) {
					j->pin_bases.hold(j->reads.bases);
					j->pin_offs.hold(j->reads.offs);
					j->pin_results.hold(j->results);
					j->pin_ops.hold(j->ops);
				}
				size_t used = 0;
				const auto tg0 = now();
				int mrc = R.paired ? urmapx_map_pe(C, j->reads.bases.data(), j->reads.offs.data(), n / 2, j->results.data(), j->ops.data(),
				                                   j->ops.size(), &used)
				                   : urmapx_map_se(C, j->reads.bases.data(), j->reads.offs.data(), n, j->results.data(), j->ops.data(),
				                                   j->ops.size(), &used);
				if (mrc != URMAPX_OK && mrc != URMAPX_E_UNSUPPORTED)
					R.fail.raise(mrc, std::string(R.paired ? "urmapx_map_pe: " : "urmapx_map_se: ") + urmapx_strerror(mrc));
				else if (R.paired && R.ftab) {
					j->info.resize(n / 2);
					mrc = urmapx_ctx_get_pair_info(C, j->info.data(), n / 2);
					if (mrc) R.fail.raise(mrc, std::string("urmapx_ctx_get_pair_info: ") + urmapx_strerror(mrc));
				}
				R.add_lane_time(&Rep::gpu_s, tg0);
			}
			mapped[(size_t)l]->push(std::move(j));
		}
		mapped[(size_t)l]->close();
	}
	void format_batch(const Job &j, std::vector<std::string> &outs, std::vector<Cnt> &cnt) {
		const bool paired = R.paired;
		const uint32_t n = j.reads.size(), units = paired ? n / 2 : n;
		const int T = R.host_threads;
		// -tags NM / MD: the store bytes under every mapped record of the batch.  Where the index keeps its host arrays the formatters read
		// them there; the command line's index lives in HBM only, so the batch's windows come back in one gather and one copy
		// (urmapx_index_fetch_spans).  ref_at[i]: where record i's window starts in `windows`; ~0: none
		std::vector<uint8_t> windows;
		std::vector<uint64_t> ref_at;
		const bool tagged = R.tagged() && R.have_sam;
		if (tagged && (R.tags & (URMAPX_TAG_NM | URMAPX_TAG_MD)) && !index_host_seq(R.I)) {
			std::vector<uint64_t> starts;
			std::vector<uint32_t> lens;
			ref_at.assign(n, ~0ull);
			uint64_t total = 0;
			for (uint32_t i = 0; i < n; ++i) {
				const urmapx_result &r = j.results[i];
				if (r.dbpos == 0xFFFFFFFFu) continue;
				const uint32_t span = ref_span(r, j.ops.data(), (unsigned)(j.reads.offs[i + 1] - j.reads.offs[i]));
				starts.push_back((uint64_t)urmapx_index_seq_offset(R.I, r.seq_index) + r.coord);
				lens.push_back(span);
				ref_at[i] = total;
				total += span;
			}
			windows.resize((size_t)total + 1);
			const int frc = urmapx_index_fetch_spans(R.I, starts.data(), lens.data(), (uint32_t)starts.size(), windows.data());
			if (frc) R.fail.raise(frc, std::string("urmapx_index_fetch_spans: ") + urmapx_strerror(frc));
		}
		auto window_of = [&](uint32_t i) -> const uint8_t * { return !ref_at.empty() && ref_at[i] != ~0ull ? windows.data() + ref_at[i] : nullptr; };
		const char *const rg_id = R.rg_line ? R.rg_id.c_str() : nullptr;
#pragma omp parallel for schedule(static, 1) num_threads(T)
		for (int t = 0; t < T; ++t) {
			std::string &out = outs[(size_t)t];
			out.clear();
			Cnt &c = cnt[(size_t)t];
			const uint32_t u0 = (uint32_t)part(units, t, T), u1 = (uint32_t)part(units, t + 1, T);
			std::vector<char> pbuf;
			for (uint32_t i = paired ? 2 * u0 : u0; i < (paired ? 2 * u1 : u1); ++i) {
				const urmapx_result &r = j.results[i];
				const uint64_t off = j.reads.offs[i];
				const unsigned L = (unsigned)(j.reads.offs[i + 1] - off);
				if (paired && R.have_sam && (i & 1) == 0) {  // a pair's two records; BAM: the host encoders (sam.cpp) write the bytes the device writes for the same read
					const uint64_t off2 = j.reads.offs[i + 1];
					const unsigned L2 = (unsigned)(j.reads.offs[i + 2] - off2);
					const size_t names = strlen(j.reads.label(i)) + strlen(j.reads.label(i + 1));
					// (with fields: an MD text is at most two bytes a reference base, and the path says how many more of those than read bases)
					pbuf.resize(names + (R.bam ? 2 * (size_t)(L + L2) + 4 * ((size_t)r.path_nops + j.results[i + 1].path_nops) : 3 * (size_t)(L + L2)) + 2048 +
					            (tagged ? 2 * ((size_t)L + L2) + 2 * R.rg_id.size() + 1024 : 0));
					urmapx_tag_options TO{R.tags, rg_id, {window_of(i), window_of(i + 1)}};
					size_t k = (R.bam ? urmapx_bam_pe_tags : urmapx_sam_pe_tags)(R.I, &j.results[i], &j.results[i + 1], j.ops.data(), j.reads.label(i),
					                                                         j.reads.bases.data() + off, j.reads.quals.data() + off, L, j.reads.label(i + 1),
					                                                         j.reads.bases.data() + off2, j.reads.quals.data() + off2, L2, tagged ? &TO : nullptr, pbuf.data(), pbuf.size());
					if (tagged && k == 0) {  // (deletions longer than the allowance, or no store bytes)
						pbuf.resize(pbuf.size() + 2 * ((size_t)ref_span(j.results[i], j.ops.data(), L) + ref_span(j.results[i + 1], j.ops.data(), L2)));
						k = (R.bam ? urmapx_bam_pe_tags : urmapx_sam_pe_tags)(R.I, &j.results[i], &j.results[i + 1], j.ops.data(), j.reads.label(i),
						                                                      j.reads.bases.data() + off, j.reads.quals.data() + off, L, j.reads.label(i + 1),
						                                                      j.reads.bases.data() + off2, j.reads.quals.data() + off2, L2, &TO, pbuf.data(), pbuf.size());
						if (k == 0) R.fail.raise(URMAPX_E_ARG, "optional fields: the index has no sequence store to compare with");
					}
					if (R.bam && k == URMAPX_BAM_LONG_NAME) R.fail.raise(URMAPX_E_FORMAT, bam_long_name(strlen(j.reads.label(i)) >= strlen(j.reads.label(i + 1)) ? j.reads.label(i) : j.reads.label(i + 1)));
					else out.append(pbuf.data(), k);
				} else if (!paired && R.bam) {
					const size_t at = out.size();
					if (!append_bam_record(out, R.I, r, j.ops.data(), 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, j.reads.label(i),
					                       j.reads.bases.data() + off, j.reads.quals.data() + off, L))
						R.fail.raise(URMAPX_E_FORMAT, bam_long_name(j.reads.label(i)));
					else if (tagged && !append_record_tags(out, at, true, R.I, r, j.ops.data(), j.reads.bases.data() + off, L, R.tags, rg_id, window_of(i)))
						R.fail.raise(URMAPX_E_ARG, "optional fields: the index has no sequence store to compare with");
				} else if (!paired && R.have_sam) {
					const size_t at = out.size();
					append_sam_record(out, R.I, r, j.ops.data(), 0, "*", 0xFFFFFFFFu, 0, j.reads.label(i),
					                  j.reads.bases.data() + off, j.reads.quals.data() + off, L);
					if (tagged && !append_record_tags(out, at, false, R.I, r, j.ops.data(), j.reads.bases.data() + off, L, R.tags, rg_id, window_of(i)))
						R.fail.raise(URMAPX_E_ARG, "optional fields: the index has no sequence store to compare with");
				}
				// HitStats counters (output1.cpp:20-30)
				if (r.status) ++c.unsupported;
				if (r.dbpos == 0xFFFFFFFFu) ++c.nohit;
				else if (r.mapq >= R.minq) ++c.accept;
				else ++c.reject;
			}
			c.text = out.size();
			if (R.bgzf && !bgzf_members(out)) R.fail.raise(URMAPX_E_NOMEM, "out of memory");
		}
	}
	// tab lines: formatted by all host threads (pair ranges), written in order
	void write_tab_lines(const Job &j) {
		const uint32_t units = j.reads.size() / 2;
		const int T = R.host_threads;
		std::vector<std::string> tabs((size_t)T);
#pragma omp parallel for schedule(static, 1) num_threads(T)
		for (int t = 0; t < T; ++t) {
			char line[4096];
			for (uint32_t u = (uint32_t)part(units, t, T); u < (uint32_t)part(units, t + 1, T); ++u) {
				const uint32_t i = 2 * u;
				const unsigned L1 = (unsigned)(j.reads.offs[i + 1] - j.reads.offs[i]), L2 = (unsigned)(j.reads.offs[i + 2] - j.reads.offs[i + 1]);
				const size_t k = urmapx_tab_pe(R.I, &j.results[i], &j.results[i + 1], &j.info[u], j.reads.label(i), L1, L2,
				                               R.have_sam ? 1 : 0, line, sizeof line);
				tabs[(size_t)t].append(line, k);
			}
		}
		for (const std::string &tb : tabs)
			if (fwrite(tb.data(), 1, tb.size(), R.ftab.get()) != tb.size()) R.fail.raise(URMAPX_E_IO, std::string("Error writing ") + R.tabout);
	}
	void formatter() {
		omp_team(R.host_threads);
		const size_t T = (size_t)R.host_threads;
		std::unique_ptr<Job> j;
		std::unique_ptr<Text> text;
		for (size_t b = 0; mapped[b % (size_t)R.n_lanes]->pop(j); ++b) {
			if (R.fail.set.load()) { recycled.push(std::move(j)); continue; }
			std::vector<Cnt> cnt(T);
			if (!text && !text_pool.try_pop(text)) text = std::make_unique<Text>();
			text->outs.resize(T);
			const auto tf0 = now();
			format_batch(*j, text->outs, cnt);
			for (const Cnt &c : cnt) {
				R.rep.mapped_q += c.accept; R.rep.mapped_lowq += c.reject; R.rep.unmapped += c.nohit; R.rep.unsupported += c.unsupported;
				R.rep.sam_text_bytes += c.text;
			}
			R.rep.reads += j->reads.size();
			R.rep.format_s += secs(tf0, now());
			if (R.have_sam) {
				std::vector<uint64_t> &at = text->at;
				at.assign(T + 1, 0);
				at[0] = R.rep.sam_file_bytes;
				for (size_t t = 0; t < T; ++t) at[t + 1] = at[t] + text->outs[t].size();
				R.rep.sam_file_bytes = at[T];
				to_flush.push(std::move(text));
			}
			if (R.ftab && R.paired) write_tab_lines(*j);
			recycled.push(std::move(j));
		}
		to_flush.close();
	}
	void flusher() {
		const int T = R.host_threads;
		std::unique_ptr<Text> x;
		while (to_flush.pop(x)) {
			const auto tw0 = now();
			if (!R.fail.set.load()) {
				if (!R.sink.reserve(x->at[(size_t)T])) R.cannot_write_sam();
				// (a pipe: the pieces one after the other; behind a piece that failed the others are refused, their offset is not the file's end)
#pragma omp parallel for schedule(static, 1) num_threads(T) if (R.sink.seekable())
				for (int t = 0; t < T; ++t) {
					const std::string &out = x->outs[(size_t)t];
					if (!R.sink.write_at(out.data(), out.size(), x->at[(size_t)t], 1)) R.cannot_write_sam();
				}
			}
			R.rep.write_s += secs(tw0, now());
			text_pool.push(std::move(x));
		}
	}
};

int map_files_impl(urmapx_index *I, const urmapx_map_options *opt, const InputRange &range, const char *fastq1, const char *fastq2,
                   const char *samout, const char *tabout, urmapx_map_report *report, char *err, size_t errcap) {
	if (err && errcap) err[0] = 0;
	if (!I || !opt || !fastq1) return URMAPX_E_ARG;
	Run R{I, *opt, range, fastq1, fastq2, samout, tabout};
	std::string msg;
	int rc = R.open(msg);
	if (!rc) {
		bool host_work = true;
		{
			TextPhase text{R};
			if (text.open_input()) {
				text.run();
				host_work = text.leaves_work();
			}
		}
		if (host_work) HostPhase{R}.run();
		rc = R.finish(report, msg);
	}
	say(err, errcap, msg);
	return rc;
}

}  // namespace

// cmd_map / cmd_map2 as a library call; with sam_shards > 1 as that many pipelines side by side, each over its part of the
// input with its own SAM file, devices and writer (the reference appends every record to one file under one lock,
// output1.cpp:10-16: one output stream is what bounds a run on several GPUs)
static int map_files_entry(urmapx_index *I, const urmapx_map_options *opt, const char *fastq1, const char *fastq2,
                           const char *samout, const char *tabout, urmapx_map_report *report, char *err, size_t errcap) {
	if (err && errcap) err[0] = 0;
	if (!I || !opt || !fastq1) return URMAPX_E_ARG;
	if (opt->bam && opt->bgzf) { say(err, errcap, "bam and bgzf together: a BAM file is always BGZF"); return URMAPX_E_ARG; }
	if (opt->tags & ~URMAPX_TAG_ALL) { say(err, errcap, "tags: bits outside URMAPX_TAG_NM | URMAPX_TAG_MD | URMAPX_TAG_AS"); return URMAPX_E_ARG; }
	if (opt->read_group) {
		char why[256];
		if (urmapx_read_group_id(opt->read_group, nullptr, 0, nullptr, 0, why, sizeof why)) { say(err, errcap, why); return URMAPX_E_ARG; }
		if (strstr(opt->read_group, "\\t")) { say(err, errcap, "read_group: the line takes real tabs here (the command line turns \\t into them)"); return URMAPX_E_ARG; }
	}
	if (opt->bam_sort) {
		const char *why = !opt->bam || !samout ? "bam_sort needs bam: it sorts the records of a BAM file" :
		                  opt->sam_shards > 1 ? "bam_sort with sam_shards: one sorted file has one index" :
		                  opt->discard_sam ? "bam_sort with discard_sam: there is nothing to sort" : nullptr;
		if (why) { say(err, errcap, why); return URMAPX_E_ARG; }
	}
	if (opt->markdup && !opt->bam_sort) { say(err, errcap, "markdup needs bam_sort: the duplicates are marked while the records are sorted"); return URMAPX_E_ARG; }
	if (opt->sort_mem && !opt->bam_sort) { say(err, errcap, "sort_mem needs bam_sort: it is the device memory the sort may take"); return URMAPX_E_ARG; }
	depth_summary().clear();
	if (opt->depth_out && !opt->bam_sort) { say(err, errcap, "depth_out needs bam_sort: the depth is taken while the records are sorted"); return URMAPX_E_ARG; }
	if (opt->depth_mapq && !opt->depth_out) { say(err, errcap, "depth_mapq needs depth_out: it is the least MAPQ of a record the depth counts"); return URMAPX_E_ARG; }
	if (opt->depth_mapq > 255) { say(err, errcap, "depth_mapq: a MAPQ is 0 .. 255"); return URMAPX_E_ARG; }
	if (opt->depth_out && samout && (!strcmp(opt->depth_out, samout) || std::string(opt->depth_out) == std::string(samout) + ".bai")) {
		say(err, errcap, "depth_out names the BAM file or its index: the depth needs a file of its own");
		return URMAPX_E_ARG;
	}
	if (opt->stats_out && !opt->bam_sort) { say(err, errcap, "stats_out needs bam_sort: the statistics are counted while the records are sorted"); return URMAPX_E_ARG; }
	if (opt->stats_out && !opt->stats_out[0]) { say(err, errcap, "stats_out needs a file name"); return URMAPX_E_ARG; }
	if (opt->stats_out && ((samout && (!strcmp(opt->stats_out, samout) || std::string(opt->stats_out) == std::string(samout) + ".bai")) ||
	                       (opt->depth_out && !strcmp(opt->stats_out, opt->depth_out)))) {
		say(err, errcap, "stats_out names the BAM file, its index or the depth file: the statistics need a file of their own");
		return URMAPX_E_ARG;
	}
	if (opt->vcf_out && !opt->bam_sort) { say(err, errcap, "vcf_out needs bam_sort: the bases are piled up while the records are sorted"); return URMAPX_E_ARG; }
	if (opt->vcf_out && !opt->vcf_out[0]) { say(err, errcap, "vcf_out needs a file name"); return URMAPX_E_ARG; }
	if (opt->vcf_out && ((samout && (!strcmp(opt->vcf_out, samout) || std::string(opt->vcf_out) == std::string(samout) + ".bai")) ||
	                     (opt->depth_out && !strcmp(opt->vcf_out, opt->depth_out)) || (opt->stats_out && !strcmp(opt->vcf_out, opt->stats_out)))) {
		say(err, errcap, "vcf_out names the BAM file, its index, the depth file or the statistics' file: the sites need a file of their own");
		return URMAPX_E_ARG;
	}
	if (opt->vcf_out && (opt->vcf_mapq > 255u || opt->vcf_baseq > 255u || opt->vcf_min_alt == 0u || opt->vcf_min_pct > 100u)) {
		say(err, errcap, "vcf_out: vcf_mapq and vcf_baseq are 0 .. 255, vcf_min_alt is 1 or more, vcf_min_pct is 0 .. 100");
		return URMAPX_E_ARG;
	}
	const int shards = opt->sam_shards > 1 ? opt->sam_shards : 1;
	if (shards == 1) return map_files_impl(I, opt, InputRange(), fastq1, fastq2, samout, tabout, report, err, errcap);
	const bool paired = fastq2 != nullptr;
	const int gpus = opt->gpus > 0 ? opt->gpus : 1;
	if (!samout) { say(err, errcap, "-samshards needs -samout (the shards are named after it)"); return URMAPX_E_ARG; }
	if (shards > 64) { say(err, errcap, "-samshards must be 1..64"); return URMAPX_E_ARG; }
	if (gpus % shards != 0 && shards % gpus != 0) { say(err, errcap, "-samshards must divide -gpus or be a multiple of it"); return URMAPX_E_ARG; }
	const int host_threads = host_threads_of(*opt);
	// plain seekable files are cut; anything else (.gz, a pipe) goes to shard 0 whole
	uint64_t fsize1 = 0, fsize2 = 0;
	const int fd1 = open_plain(fastq1, fsize1), fd2 = paired ? open_plain(fastq2, fsize2) : -1;
	const bool cut = fd1 >= 0 && (!paired || fd2 >= 0) && !getenv("URMAPX_HOST_TEXT_NO_SHARDS");
	// the cutting (and, for pairs, the line counts that place the cuts of the mates' file) belongs to the run: it is inside
	// report->seconds and reported as shard_scan_s
	const auto t_scan0 = now();
	// shard s starts at the first record start at or behind byte fsize * s / shards of the first file -- and, for pairs, at
	// the same line of the second file
	std::vector<InputRange> ranges((size_t)shards);
	std::vector<uint64_t> at((size_t)shards + 1, 0), at2((size_t)shards + 1, 0), lines((size_t)shards + 1, 0);
	at[(size_t)shards] = fsize1; at2[(size_t)shards] = fsize2;
	if (cut) {
		for (int s = 1; s < shards; ++s) {
			const uint64_t nominal = fsize1 / (uint64_t)shards * (uint64_t)s;
			uint64_t a = nominal > at[(size_t)s - 1] ? find_record_start(fd1, nominal, fsize1) : at[(size_t)s - 1];
			if (a == 0 || a < at[(size_t)s - 1]) a = fsize1;  // no record start in sight: the shard in front takes the rest
			at[(size_t)s] = a;
		}
		if (paired) {  // the mates' file is cut at the same LINES: the first file's parts are counted, the second's offsets looked up
			for (int s = 1; s < shards; ++s) lines[(size_t)s] = lines[(size_t)s - 1] + count_newlines(fd1, at[(size_t)s - 1], at[(size_t)s], host_threads);
			const std::vector<uint64_t> o2 = line_offsets(fd2, fsize2, std::vector<uint64_t>(lines.begin() + 1, lines.begin() + shards), host_threads);
			for (int s = 1; s < shards; ++s) at2[(size_t)s] = o2[(size_t)s - 1];
		}
	}
	for (int s = 0; s < shards; ++s) {
		InputRange &r = ranges[(size_t)s];
		r.header = s == 0;
		r.on = cut;
		r.lo[0] = at[(size_t)s]; r.hi[0] = at[(size_t)s + 1]; r.lo[1] = at2[(size_t)s]; r.hi[1] = at2[(size_t)s + 1];
		r.lines_before = lines[(size_t)s];
		if (cut && !paired && s > 0) {
			// single-end: nothing needs the line counts but a message about a malformed record -- the shard's reader counts then
			const std::string path = fastq1;
			const uint64_t upto = at[(size_t)s];
			r.lazy_lines = [path, upto, host_threads]() -> uint64_t {
				const int fd = open(path.c_str(), O_RDONLY);
				if (fd < 0) return 0;
				const uint64_t n = count_newlines(fd, 0, upto, host_threads);
				close(fd);
				return n;
			};
		}
	}
	if (paired && cut) ranges[(size_t)shards - 1].hi[1] = fsize2;
	if (fd1 >= 0) close(fd1);
	if (fd2 >= 0) close(fd2);
	const double scan_s = secs(t_scan0, now());
	// a shard without records: an empty file, under -bgzf the end-of-file member alone (every shard is a complete BGZF file), under
	// -bamout the header block in a member of its own in front of that (every shard is a complete BAM file)
	auto empty_shard = [&](int s) {
		if (FILE *f = fopen(shard_name(samout, s).c_str(), "wb")) {
			std::string eof;
			if (opt->bam) append_bam_header(eof, I, opt->cmdline, false, opt->read_group);
			if ((opt->bgzf || opt->bam) && bgzf_members(eof, 1)) (void)fwrite(eof.data(), 1, eof.size(), f);
			fclose(f);
		}
		if (tabout) create_empty(shard_name(tabout, s));
	};
	auto remove_shard = [&](int s) {
		remove(shard_name(samout, s).c_str());
		if (tabout) remove(shard_name(tabout, s).c_str());
	};
	if (!cut) {
		// Input that cannot be cut (.gz, BGZF, a pipe): ONE pipeline with all the devices and lanes the caller gave writes shard 0, the
		// other shards are empty files -- `cat` of the shards is still the one file.  (Until round 4 shard 0 ran on gpus / shards of
		// the devices: `-gpus 8 -samshards 8 reads.fq.gz` mapped the whole file on one GPU.)
		urmapx_map_options o = *opt;
		o.sam_shards = 0;
		const std::string sam0 = shard_name(samout, 0), tab0 = tabout ? shard_name(tabout, 0) : std::string();
		const int rc1 = map_files_impl(I, &o, InputRange(), fastq1, fastq2, sam0.c_str(), tabout ? tab0.c_str() : nullptr, report, err, errcap);
		if (rc1 == URMAPX_OK || rc1 == URMAPX_E_UNSUPPORTED)
			for (int s = 1; s < shards; ++s) empty_shard(s);
		else remove_shard(0);
		if (report) report->shards = shards;
		return rc1;
	}
	// devices: shard s takes gpus / shards of them, or shares device s mod gpus
	const int per = gpus >= shards ? gpus / shards : 1;
	// one replica of the index on the first device of every shard (a shard with several devices makes the others' itself)
	std::vector<urmapx_index *> replicas((size_t)gpus, nullptr);
	int rc = urmapx_index_upload(I, phys_device(*opt, 0));
	replicas[0] = I;
	for (int g = per; g < gpus && !rc; g += per) rc = urmapx_index_replicate(I, phys_device(*opt, g), &replicas[(size_t)g]);
	auto release = [&]() { for (int g = 1; g < gpus; ++g) urmapx_index_close(replicas[(size_t)g]); };
	if (rc) { say(err, errcap, std::string("Uploading index to the GPU: ") + urmapx_strerror(rc)); release(); return rc; }
	std::vector<urmapx_map_report> reps((size_t)shards);
	std::vector<int> rcs((size_t)shards, 0);
	std::vector<std::string> errs((size_t)shards);
	std::vector<std::thread> th;
	const auto t0 = now();
	for (int s = 0; s < shards; ++s)
		th.emplace_back([&, s] {
			urmapx_map_options o = *opt;
			o.sam_shards = 0;
			o.gpus = per;
			// pipelines that share a device share its lanes too: K contexts per device in all, as in a run of one pipeline
			if (shards > gpus) o.streams = std::max(1, (opt->streams > 0 ? opt->streams : 2) * gpus / shards);
			const int g0 = gpus >= shards ? s * per : s % gpus;
			o.first_gpu = opt->first_gpu + g0;
			o.host_threads = std::max(2, host_threads / shards);
			const std::string sam = shard_name(samout, s), tab = tabout ? shard_name(tabout, s) : std::string();
			char e[512];
			e[0] = 0;
			memset(&reps[(size_t)s], 0, sizeof reps[(size_t)s]);
			const InputRange &r = ranges[(size_t)s];
			if (r.lo[0] >= r.hi[0]) { empty_shard(s); return; }  // nothing left for this shard (fewer records than shards)
			rcs[(size_t)s] = map_files_impl(replicas[(size_t)g0], &o, r, fastq1, fastq2, sam.c_str(), tabout ? tab.c_str() : nullptr, &reps[(size_t)s], e, sizeof e);
			errs[(size_t)s] = e;
		});
	for (auto &t : th) t.join();
	double wall = secs(t0, now());
	{
		double b = 0, e = 0;
		for (const InputRange &r : ranges)
			if (r.t_end > 0) { b = b == 0 ? r.t_begin : std::min(b, r.t_begin); e = std::max(e, r.t_end); }
		if (e > b) wall = e - b;
	}
	wall += scan_s;
	release();
	int out_rc = URMAPX_OK;
	for (int s = 0; s < shards; ++s)
		if (rcs[(size_t)s] && rcs[(size_t)s] != URMAPX_E_UNSUPPORTED && out_rc == URMAPX_OK) { out_rc = rcs[(size_t)s]; say(err, errcap, errs[(size_t)s]); }
	if (out_rc != URMAPX_OK)  // a failed run leaves no partial shard files behind (the first error is the one reported)
		for (int s = 0; s < shards; ++s) remove_shard(s);
	if (report) {
		memset(report, 0, sizeof *report);
		for (const urmapx_map_report &r : reps) {
			for (auto f : kReportCounts) report->*f += r.*f;
			for (auto f : kReportTimes) report->*f += r.*f;
			report->lanes += r.lanes; report->host_threads += r.host_threads;
			report->write_threads = std::max(report->write_threads, r.write_threads);
			report->text_on_device |= r.text_on_device;
			if (r.medium[0]) memcpy(report->medium, r.medium, sizeof report->medium);
			if (r.placement[0]) {
				const size_t have = strlen(report->placement);
				snprintf(report->placement + have, sizeof report->placement - have, "%s%s", have ? " | " : "", r.placement);
			}
		}
		report->seconds = wall;
		report->shards = shards;
		report->shard_scan_s = scan_s;
	}
	if (out_rc != URMAPX_OK) return out_rc;
	return report && report->unsupported ? URMAPX_E_UNSUPPORTED : URMAPX_OK;
}

extern "C" int urmapx_map_files(urmapx_index *I, const urmapx_map_options *opt, const char *fastq1, const char *fastq2,
                                const char *samout, const char *tabout, urmapx_map_report *report, char *err, size_t errcap) {
	// what the call spent in allocation calls (all of its threads): device arrays of the lanes' contexts, page-locked chunk buffers
	AllocClock &ac = alloc_clock();
	const uint64_t ns0[2] = {ac.ns[0].load(), ac.ns[1].load()}, c0[2] = {ac.calls[0].load(), ac.calls[1].load()};
	const int rc = map_files_entry(I, opt, fastq1, fastq2, samout, tabout, report, err, errcap);
	if (report) {
		report->alloc_dev_s = (double)(ac.ns[0].load() - ns0[0]) * 1e-9; report->alloc_pinned_s = (double)(ac.ns[1].load() - ns0[1]) * 1e-9;
		report->alloc_dev_calls = (uint32_t)(ac.calls[0].load() - c0[0]); report->alloc_pinned_calls = (uint32_t)(ac.calls[1].load() - c0[1]);
	}
	return rc;
}
extern "C" const char *urmapx_map_depth_summary(void) { return depth_summary().c_str(); }
extern "C" void urmapx_host_pool_trim(void) {
	LanePool::get().purge(nullptr);
	HostPool::get().trim();
}
namespace urx {
void lane_pool_purge(const urmapx_index *I) { LanePool::get().purge(I); }
}
