// ngm_cli.cpp -- `ngm-hip`: NextGenMap-compatible command line over the C ABI (include/ngm_pipeline.h).
//
// Mirrors what ngm-core does around its hot path:
//   option names / defaults          src/config/Options.h:13-105, src/config/Config.cpp:381-557
//   read parsing                     src/parser/IParser.h:59-121 (upper-case, non-ACGT -> N, truncate to qry_max_len-1)
//   parameter estimation             src/ReadProvider.cpp:163-394 (qry_max_len, corridor, sensitivity)
//   output filter                    src/writer/GenericReadWriter.h:190-254 (min_identity, min_residues), min_mq
//   SAM header / records             src/writer/SAMWriter.cpp:17-84, :98-228, :312-373
//   batch hand-out to workers        src/NGM.cpp:232-279 (GetNextReadBatch under a mutex), src/CS.cpp:440-456 (-g: threads -> devices)
//   buffered, ordered output         src/writer/GenericReadWriter.h:190-304 (20 MB buffer, flushed under the output lock)
// Everything heavy (index, candidate search, score, align) happens on the GPU behind ngm_mapper_*.
// Single-end and paired-end (-p -q interleaved, --qry1/--qry2), FASTA / FASTQ (plain, .gz), SAM and BAM input, --affine, -n/--strata, SAM and BAM (--bam) output, one or
// several GPUs (-g 0,1,...), and --argos (ScoreWriter's lines, src/writer/ScoreWriter.cpp: every scored candidate of a read, ordered on the
// GPU -- single-end only, see ngm_mapper_map_argos), bisulfite (--bs-mapping) and SLAM-seq (--slam-seq) mapping, -5/--trim5 and --max-polya
// (csrc/read_trim.h), and --sort (ours, with --bam: the records of the whole run stay in GPU memory, are sorted there into coordinate order and
// written as the sorted BAM plus <output>.bai, csrc/bam_sort.cpp; not with --argos, --shard, --shard-output, NGM_HIP_BAM_ZLIB=1, nor a
// contig above 2^29 bases; with --markdup duplicate records get flag 0x400 there before the sort, csrc/markdup.h), and --coverage FILE (ours: the per-base depth of the run's mapped primary records as bedGraph, counted and turned into text on the
// GPU, csrc/coverage.cpp; not with --argos, --shard, --shard-output, nor FILE = the output), and --snp FILE with --snp-min-cov / --snp-min-frac /
// --snp-min-qual (ours: the mismatch pileup of the same records and its single-base substitution calls as VCF, counted and turned into text on the GPU,
// csrc/snp.cpp; not with --argos, --shard, --shard-output, --bs-mapping, --vcf, nor FILE = the output or the --coverage file), and --count BED --count-out FILE
// with --count-min-qual (ours: T>C conversion counts of the same records per region of the BED file, counted and summed on the GPU, the positions --snp calls
// left out, csrc/count.cpp; not with --argos, --shard, --shard-output, --bs-mapping, nor FILE = another output), and --methyl FILE with --methyl-context,
// --methyl-min-qual, --methyl-min-depth (ours, with --bs-mapping: the per-cytosine methylation calls of the same records as Bismark's cytosine report, counted and
// turned into text on the GPU, csrc/methyl.cpp; not with --argos, --shard, --shard-output, nor FILE = the output or the --coverage file).  Not supported (rejected loudly): --vcf with --bs-mapping, --max-polya with --argos or --vcf, --config.
//
// Pass 2 is a pipeline, not a loop:
//   splitter (1 thread)   cuts the input into batches: for plain 4-line FASTQ it only counts line ends in the mapped file
//                         (record boundaries every 1 024 reads), for gz / FASTA / multi-line input it is the serial kseq-style
//                         reader (inflate is one stream; that is the bound of such input, as in the reference);
//   workers               `--workers` per GPU (default 2), each owning an ngm_mapper like a NextGenMap CS thread owns its
//                         IAlignment: parse its batch into a page-locked row buffer (pool threads, zero-copy names / qualities),
//                         map it on its GPU, format the SAM text (pool threads) -- while one worker's batch is on the GPU the
//                         others parse and format;
//   writer (1 thread)     batches in input order, large writes.
// Paired-end tie-breaks see the same running mean insert size as `ngm -t 1` (ngm_pair_state: batches take turns for that
// part only), so the output does not depend on the number of workers or GPUs.
//
// One translation unit in four files: cli_options.h (options and their refusals), cli_input.h (readers, record indexes, batches),
// cli_format.h (the host formatter: records -> SAM / BAM) and this one -- the run, as the stages of `struct Run` in main()'s order.
#include <dlfcn.h>
#include <malloc.h>
#include <poll.h>
#include <signal.h>
#include <sys/resource.h>
#include <sys/sendfile.h>
#include <sys/time.h>
#include <sys/wait.h>
#include <ucontext.h>

#include <chrono>
#include <map>

#include "cli_format.h"
#include "cli_input.h"
#include "cli_options.h"
#include "count.h"

using namespace ngm::cli;

namespace {

// NGM_HIP_PROFILE=file: a sampling profile of the host side without any tool installed -- ITIMER_PROF ticks (1 kHz of process
// CPU time, delivered to whichever thread is running), the interrupted instruction's address per tick, written as
// "module offset count" lines at exit (resolve with addr2line -e <module> -f -C -i <offset>).
namespace prof {
constexpr int kSlots = 1 << 16;
std::atomic<uintptr_t> g_ip[kSlots];
std::atomic<unsigned> g_n{0};
void on_tick(int, siginfo_t *, void *uc) {
	const unsigned at = g_n.fetch_add(1, std::memory_order_relaxed);
	if (at < (unsigned) kSlots) g_ip[at].store((uintptr_t) ((ucontext_t *) uc)->uc_mcontext.gregs[REG_RIP], std::memory_order_relaxed);
}
void start() {
	struct sigaction sa;
	memset(&sa, 0, sizeof(sa));
	sa.sa_sigaction = on_tick;
	sa.sa_flags = SA_SIGINFO | SA_RESTART;
	sigaction(SIGPROF, &sa, nullptr);
	struct itimerval tv = {{0, 1000}, {0, 1000}};
	setitimer(ITIMER_PROF, &tv, nullptr);
}
void dump(const char *path) {
	struct itimerval off = {{0, 0}, {0, 0}};
	setitimer(ITIMER_PROF, &off, nullptr);
	const unsigned n = std::min(g_n.load(), (unsigned) kSlots);
	std::map<std::pair<std::string, uintptr_t>, unsigned> hist;
	for (unsigned i = 0; i < n; ++i) {
		const uintptr_t ip = g_ip[i].load();
		Dl_info di;
		if (dladdr((void *) ip, &di) && di.dli_fname) hist[{di.dli_fname, ip - (uintptr_t) di.dli_fbase}] += 1;
		else hist[{"?", ip}] += 1;
	}
	if (FILE *f = fopen(path, "w")) {
		fprintf(f, "# %u samples (1 ms of process CPU time each)\n", g_n.load());
		for (const auto &e : hist) fprintf(f, "%s 0x%lx %u\n", e.first.first.c_str(), (unsigned long) e.first.second, e.second);
		fclose(f);
	}
}
}  // namespace prof

}  // namespace

// `-g a,b,... --shard-output`: one process per GPU.  Child k runs this program again with `--device <k-th GPU> --shard
// k/N -o <out>.shard<k>`: its own reference copy in that GPU's HBM, its own reader, workers, paired-end state and writer -- nothing is
// shared, so N GPUs write N files at once instead of queueing behind one writer.  Shard 0 carries the header; the pieces are
// appended to <out> in shard order (in-kernel copies) unless --keep-shards asks for `cat <out>.shard*` to be left to the caller.
int run_sharded(int argc, char **argv, const Opts &o) {
	const int N = (int) o.devices.size();
	std::vector<pid_t> kids;
	std::vector<std::string> parts;
	for (int k = 0; k < N; ++k) parts.push_back(o.out + ".shard" + std::to_string(k));
	// cold cache: ONE process builds the index and writes the cache files (this program with the reference only), then the shards load
	// them -- not N builds of the same index, N times the host memory, all writing the same two files
	{
		const std::string enc = o.ref + "-enc.2.ngm", ht = o.ref + "-ht-" + std::to_string(o.kmer) + "-" + std::to_string(o.bs_mapping ? 0 : o.kmer_skip) + ".3.ngm";
		// (a reference directory that cannot be written gets no cache either way: every shard then builds its own index in memory, and
		// a build in front of them would only be one more)
		std::string dir = o.ref;
		const size_t slash = dir.find_last_of('/');
		dir = slash == std::string::npos ? "." : slash == 0 ? "/" : dir.substr(0, slash);
		if (!o.skip_save && access(dir.c_str(), W_OK) == 0 && (access(enc.c_str(), R_OK) != 0 || access(ht.c_str(), R_OK) != 0)) {
			info("MAIN", "No index cache next to the reference: building it once before the shard processes start");
			const pid_t pid = fork();
			if (pid < 0) die("fork failed");
			if (pid == 0) {
				std::vector<std::string> a = {argv[0], "-r", o.ref, "-k", std::to_string(o.kmer), "--kmer-skip", std::to_string(o.kmer_skip), "--device", std::to_string(o.devices[0])};
				if (o.bs_mapping) a.push_back("--bs-mapping");
				std::vector<char *> av;
				for (std::string &x : a) av.push_back(&x[0]);
				av.push_back(nullptr);
				execv("/proc/self/exe", av.data());
				_exit(127);
			}
			int st = 0;
			if (waitpid(pid, &st, 0) != pid || !WIFEXITED(st) || WEXITSTATUS(st) != 0) die("building the index failed (its messages are above)");
		}
	}
	// The one collective of the path: every shard's int64[8] statistics, summed.  The shards hand their vectors to this
	// process over a pipe each -- that sum is printed in any case -- and, on distinct GPUs, also run the ncclAllReduce among themselves
	// (RCCL over xGMI; the communicator id made here travels in their environment).
	bool distinct = true;
	for (int a = 0; a < N; ++a) for (int b = a + 1; b < N; ++b) if (o.devices[a] == o.devices[b]) distinct = false;
	if (distinct && !getenv("NGM_HIP_NO_RCCL")) {
		char hex[257];
		if (ngm_stats_unique_id(hex) == 0) setenv("NGM_HIP_RCCL_ID", hex, 1);
		else info("MAIN", std::string("note: no RCCL all-reduce of the statistics (") + ngm_pipeline_last_error() + "); summing the shards' vectors here");
	} else unsetenv("NGM_HIP_RCCL_ID");
	std::vector<int> stat_rd(N, -1);
	for (int k = 0; k < N; ++k) {
		int pfd[2];
		if (pipe(pfd) != 0) die("pipe failed");
		stat_rd[k] = pfd[0];
		const pid_t pid = fork();
		if (pid < 0) die("fork failed");
		if (pid == 0) {
			for (int j = 0; j <= k; ++j) close(stat_rd[j]);
			std::vector<std::string> a(argv, argv + argc);
			a.push_back("--stats-fd"); a.push_back(std::to_string(pfd[1]));
			a.push_back("--device"); a.push_back(std::to_string(o.devices[k]));
			a.push_back("--shard"); a.push_back(std::to_string(k) + "/" + std::to_string(N));
			a.push_back("-o"); a.push_back(parts[k]);
			std::vector<char *> av;
			for (std::string &x : a) av.push_back(&x[0]);
			av.push_back(nullptr);
			execv("/proc/self/exe", av.data());
			_exit(127);
		}
		close(pfd[1]);
		kids.push_back(pid);
	}
	// The shards' vectors (64 bytes each, written when a shard is done) and their exit codes, as they come.  A shard that fails must not
	// leave the others -- and this process -- waiting: on distinct GPUs they sit in ncclCommInitRank / ncclAllReduce, which have no timeout
	// and wait for EVERY rank.  So the pipes are polled, the children reaped as they exit, and the first failure ends the rest.
	long long total[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	int got = 0;
	bool ok = true;
	{
		std::vector<int64_t> vec((size_t) N * 8, 0);
		std::vector<size_t> have(N, 0);
		std::vector<bool> open_fd(N, true), alive(N, true);
		int n_alive = N, n_open = N;
		auto end_the_others = [&] { for (int k = 0; k < N; ++k) if (alive[k]) kill(kids[k], SIGTERM); };
		while (n_alive > 0 || n_open > 0) {
			std::vector<struct pollfd> pf;
			std::vector<int> which;
			for (int k = 0; k < N; ++k) if (open_fd[k]) { struct pollfd x; x.fd = stat_rd[k]; x.events = POLLIN; x.revents = 0; pf.push_back(x); which.push_back(k); }
			if (!pf.empty()) (void) poll(pf.data(), (nfds_t) pf.size(), 200);
			else usleep(20000);
			for (size_t j = 0; j < pf.size(); ++j) {
				if (!(pf[j].revents & (POLLIN | POLLHUP | POLLERR))) continue;
				const int k = which[j];
				const ssize_t r = have[k] < 64 ? read(stat_rd[k], (char *) &vec[(size_t) k * 8] + have[k], 64 - have[k]) : 0;
				if (r > 0) have[k] += (size_t) r;
				if (r <= 0 || have[k] == 64) {   // (end of file, or the vector is complete)
					if (r <= 0 || (pf[j].revents & POLLHUP)) { close(stat_rd[k]); open_fd[k] = false; --n_open; }
				}
			}
			for (;;) {
				int st = 0;
				const pid_t pid = waitpid(-1, &st, WNOHANG);
				if (pid <= 0) break;
				for (int k = 0; k < N; ++k) if (alive[k] && kids[k] == pid) {
					alive[k] = false; --n_alive;
					if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) { if (ok) end_the_others(); ok = false; }
				}
			}
			if (n_alive == 0) for (int k = 0; k < N; ++k) if (open_fd[k]) {   // (every writer has gone: what is in the pipes is all there will be)
				const ssize_t r = have[k] < 64 ? read(stat_rd[k], (char *) &vec[(size_t) k * 8] + have[k], 64 - have[k]) : 0;
				if (r > 0) have[k] += (size_t) r;
				close(stat_rd[k]); open_fd[k] = false; --n_open;
			}
		}
		for (int k = 0; k < N; ++k) if (have[k] == 64) { ++got; for (int j = 0; j < 8; ++j) total[j] += vec[(size_t) k * 8 + j]; }
	}
	if (!ok) die("a shard process failed (its messages are above)");
	if (got == N) {
		infof("MAIN", "Done, %d shards summed (%lld reads mapped (%.2f%%), %lld reads not mapped, %lld lines written; %lld reads; %lld pairs with both mates mapped, %lld of them broken, mean insert size %.1f)",
				N, total[1], total[0] ? 100.0 * total[1] / total[0] : 0.0, total[2], total[3], total[0], total[4], total[5], total[7] > 0 ? (double) total[6] / (double) total[7] : 0.0);
	} else info("MAIN", "warning: not every shard handed over its statistics");
	if (o.keep_shards) { info("MAIN", "Shards written: " + parts[0] + " .. " + parts.back() + " (concatenate in this order)"); return 0; }
	const auto t0 = std::chrono::steady_clock::now();
	if (rename(parts[0].c_str(), o.out.c_str()) != 0) die("cannot rename " + parts[0]);
	const int out_fd = ::open(o.out.c_str(), O_WRONLY);   // (not O_APPEND: sendfile refuses such a target)
	if (out_fd < 0 || lseek(out_fd, 0, SEEK_END) < 0) die("cannot append to " + o.out);
	for (int k = 1; k < N; ++k) {
		const int in_fd = ::open(parts[k].c_str(), O_RDONLY);
		struct stat st;
		if (in_fd < 0 || fstat(in_fd, &st) != 0) die("cannot read " + parts[k]);
		off_t left = st.st_size;
		while (left > 0) {
			const ssize_t w = sendfile(out_fd, in_fd, nullptr, (size_t) std::min<off_t>(left, (off_t) 1 << 30));
			if (w <= 0) die("write error on " + o.out);
			left -= w;
		}
		close(in_fd);
		unlink(parts[k].c_str());
	}
	if (close(out_fd) != 0) die("write error on " + o.out);
	infof("MAIN", "%d shards appended to the output in %.3f s", N, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
	return 0;
}

namespace {

long long us_since(std::chrono::steady_clock::time_point t0) { return (long long) std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count(); }
double span_s(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b = std::chrono::steady_clock::now()) { return std::chrono::duration<double>(b - a).count(); }
// adds the thread time of a pool task to a stage's counter when the task ends
struct CpuTime { std::atomic<long long> &a; std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now(); ~CpuTime() { a += us_since(t); } };

// ---- who makes the records: decided once, from the options and the environment -------------------------------------------
// SAM text on the GPU (csrc/sam_device.h) for plain SAM output with one alignment per read; BAM and -n > 1 are formatted here
// --bam: the records and their BGZF blocks are written by the GPU as well (sam_device.h's BAM mode + bgzf_device.h), SLAM-seq tags
// included; with -n > 1 or --broken-pairs the records are formatted here and only the blocks come from the GPU
// (NGM_HIP_BAM_HOST_RECORDS=1 forces that; NGM_HIP_BAM_ZLIB=1: records here, zlib level 6 on the pool -- the round-3 path)
struct OutputRoute { bool gpu_bam, gpu_sam, gpu_bgzf; int topn; };
OutputRoute output_route(const Opts &o) {
	OutputRoute r;
	r.topn = o.paired ? 1 : o.topn;
	r.gpu_bam = o.bam && !getenv("NGM_HIP_BAM_ZLIB") && !getenv("NGM_HIP_BAM_HOST_RECORDS");
	r.gpu_sam = o.argos || ((!o.bam || r.gpu_bam) && r.topn == 1 && !o.broken_pairs && !getenv("NGM_HIP_HOST_SAM"));   // (--argos: its lines only come from the GPU)
	r.gpu_bgzf = o.bam && !r.gpu_sam && !getenv("NGM_HIP_BAM_ZLIB");
	return r;
}

struct TextBuf { char *p; size_t cap; };
struct Worker { ngm_mapper *m = nullptr; char *rows = nullptr; size_t rows_cap = 0; std::vector<ngm_hit> hits; std::vector<char> cig, md;
	char *qrows = nullptr, *names = nullptr; size_t names_cap = 0; ngm_sam_read *meta = nullptr;
	uint16_t *polya = nullptr; size_t polya_cap = 0;   // --max-polya: bases cut per read, for the GPU writer's XA:i (page-locked like meta; 2 bytes per read)
	ngm_bgzf *bz = nullptr; char *bam_raw = nullptr, *bam_out = nullptr; size_t bam_raw_cap = 0, bam_out_cap = 0; };

// ---- page-locked buffers: what every worker needs for batches of `batch` reads of up to q - 1 bases, and the text pool ------------
// Page-locked memory is slow to get (~0.1 s per 150 MB, ~0.9 GB for two workers): everything at once, each piece on a thread of its own.
struct Pinned {
	struct W { char *rows = nullptr, *qrows = nullptr, *names = nullptr; ngm_sam_read *meta = nullptr; char *bam_raw = nullptr, *bam_out = nullptr; };
	std::thread th;
	int q = 0, batch = 0;
	bool bam = false;   // the GPU BGZF route: a batch's records and its blocks per worker, instead of rows and text
	size_t bam_raw_cap = 0, bam_out_cap = 0;
	std::vector<TextBuf> text;
	std::vector<W> w;
	~Pinned() { join(); }
	void join() { if (th.joinable()) th.join(); }
	void request(int batch_reads, int q_, const OutputRoute &route, size_t n_workers) {   // returns at once: join() waits for the memory
		q = q_; batch = batch_reads; bam = route.gpu_bgzf;
		if (!bam) text.assign(n_workers + 2, TextBuf{nullptr, 0});
		w.assign(n_workers, W());
		// (--bam: a batch's records -- 36 bytes + name + CIGAR + 1.5 bytes per base + tags each -- and its BGZF blocks)
		bam_raw_cap = (size_t) batch * ((size_t) 2 * q + 224) + (1u << 20);
		bam_out_cap = ngm_bgzf_bound(bam_raw_cap);
		th = std::thread([this] {
			const size_t cap = (size_t) batch * ((size_t) 2 * q + 288) + (1u << 20);
			std::vector<std::thread> alloc;
			for (TextBuf &t : text) alloc.emplace_back([&t, cap] { t.p = (char *) ngm_host_alloc(cap); t.cap = t.p ? cap : 0; });
			if (bam) for (W &x : w) {
				alloc.emplace_back([&x, this] { x.bam_raw = (char *) ngm_host_alloc(bam_raw_cap); });
				alloc.emplace_back([&x, this] { x.bam_out = (char *) ngm_host_alloc(bam_out_cap); });
			}
			else for (W &x : w) alloc.emplace_back([&x, this] {
				const size_t rows = (size_t) batch * q;
				x.rows = (char *) ngm_host_alloc(rows); x.qrows = (char *) ngm_host_alloc(rows);
				x.meta = (ngm_sam_read *) ngm_host_alloc((size_t) batch * sizeof(ngm_sam_read));
				x.names = (char *) ngm_host_alloc((size_t) batch * 32);
			});
			for (auto &t : alloc) t.join();
		});
	}
	bool complete() const {   // the rows of every worker and the text pool
		bool ok = !bam;
		for (const TextBuf &t : text) ok = ok && t.p;
		for (const W &x : w) ok = ok && x.rows && x.qrows && x.meta && x.names;
		return ok;
	}
	void release() {
		for (const TextBuf &t : text) ngm_host_free(t.p);
		for (const W &x : w) { ngm_host_free(x.rows); ngm_host_free(x.qrows); ngm_host_free(x.meta); ngm_host_free(x.names); ngm_host_free(x.bam_raw); ngm_host_free(x.bam_out); }
		text.clear(); w.clear();
	}
};

// A batch that ends before its map call must still pass its turn in the paired-end statistics on (ngm_pair_state: batches take turns, and
// every later batch waits for this one): an empty call does that.  Armed when a batch is taken, disarmed where a map call has run.
struct PairTurn {
	ngm_mapper *m; bool armed;
	~PairTurn() { if (armed) (void) ngm_mapper_map_pe(m, 0, nullptr, nullptr, nullptr, nullptr); }
};

// ---- one run: what its threads share, and its stages in the order main() runs them -------------------------------------------------
struct Run {
	using Clock = std::chrono::steady_clock;
	Opts o;
	Clock::time_point t_process, t_input, t_indexed, t_estimated, t_start;
	int in_format = ngm::bamin::kFastx;
	ngm_stats_comm *stats_comm = nullptr;
	std::string stats_comm_error;
	std::thread stats_comm_thread, estimate_thread;
	OutputRoute route{};
	Pinned pinned;
	ngm_ref_params rp{};
	ngm_ref *ref = nullptr;
	// the input and what the scan of it found
	std::string first_input, path0, path1;
	MappedFile mf0, mf1;
	bool plain = false;
	int batch_reads = 0, per_file_reads = 0, sub_step = kSub, q = 0, avg_len = 0;
	FastqIndex ix0, ix1;
	size_t count = 0, total_seqs = 0;
	std::vector<Read> sample;
	ngm_mapper_params mp{};
	// the output, the mappers and the side outputs
	int out_fd = -1;
	uint64_t out_off = 0;
	std::vector<std::string> contig_names;
	std::vector<uint64_t> contig_lens;
	std::vector<ngm_ref *> refs;
	ngm_pair_state *pair_state = nullptr;
	std::vector<Worker> workers;
	ngm_bam_sort *sorter = nullptr;
	ngm_coverage *coverage = nullptr;
	ngm_snp *snp = nullptr;
	ngm_count *counter = nullptr;
	ngm_methyl *methyl = nullptr;   // --methyl: the methylation counters, beside the first GPU's resident reference
	std::vector<ngm::cnt::Region> count_regions;   // --count: the BED file's regions, read before any GPU work
	std::vector<std::string> count_names;          // ... and the contigs they were checked against (the FASTA's, as the reference will hold them)
	std::vector<uint32_t> count_lens;
	FILE *coverage_file = nullptr, *snp_file = nullptr, *count_file = nullptr, *methyl_file = nullptr;
	HostFormatter fmt;
	std::atomic<uint64_t> pair_stat[3];   // AlignmentBuffer::WriteRead's pair counters, summed over the run (the GPU formatter counts the same: ngm_mapper_last_pair_stats)
	std::atomic<bool> cov_failed{false}, snp_failed{false}, count_failed{false}, methyl_failed{false};   // an ngm_coverage_add / ngm_snp_add / ngm_count_add of a formatted range failed: the run fails behind its batch
	// the pipeline
	std::unique_ptr<BoundedQueue<std::unique_ptr<Batch>>> q_in;
	std::mutex out_mu, fail_mu, text_mu, spare_mu;
	std::condition_variable out_cv, text_cv;
	std::map<uint64_t, std::unique_ptr<Batch>> out_ready;
	std::atomic<uint64_t> next_write{0};   // the batch the writer waits for (written under out_mu)
	bool workers_done = false;
	std::atomic<bool> failed{false};
	std::string fail_msg;
	// The formatted text of a batch (~100 MB in MB-sized pieces) and its record views are recycled instead of freed: fresh memory
	// means page faults from 64 threads at once, and those serialise on the address-space lock.
	std::vector<std::vector<std::string>> spare_chunks;
	std::vector<std::vector<Rec>> spare_recs;
	// GPU-formatted text: page-locked buffers that travel worker -> writer -> pool.  Their number bounds the formatted text in
	// flight (a slow output file then stalls the workers instead of piling the output up in memory)
	std::vector<TextBuf> text_free;
	size_t text_cap0 = 0;
	std::atomic<long long> t_gpu_us{0}, t_sam_gpu_us{0}, t_bgzf_gpu_us{0}, t_bgzf_call_us{0};  // t_gpu_us: HIP-event time of the mapping kernels, summed over the batches
	std::atomic<long long> t_wait_us{0}, t_parse_us{0}, t_map_us{0}, t_format_us{0}, t_format_cpu_us{0}, t_parse_cpu_us{0}, t_write_us{0}, t_write_cpu_us{0};
	std::atomic<unsigned long long> bgzf_in_bytes{0}, bgzf_out_bytes{0};
	size_t n_total = 0, n_mapped = 0, n_written = 0, n_read = 0;   // (n_read: records of the batches; n_total: reads the writer counted as mapped or unmapped)
	struct timespec cpu0;
	struct rusage ru0;

	Run() { for (auto &x : pair_stat) x = 0; }
	~Run() { if (estimate_thread.joinable()) estimate_thread.join(); }
	// before the pipeline
	void read_count_regions(); void refuse_by_input_format(); void join_communicator(); void request_pinned_early(); void load_reference(); void scan_input();
	void run_estimate(ngm_mapper_params ep, float &sens, bool &estimated, bool logged_only); void estimate_sensitivity();
	void write_header(); void create_mappers_and_side_outputs(); void setup_formatter(); void take_pinned();
	// the pipeline's threads
	void split_plain(); void split_serial(); void splitter_main(); void worker_main(Worker &w); void writer_main();
	bool parse_batch(Worker &w, Batch &b); void check_mate_names(const Batch &b);
	void gpu_text_route(Worker &w, std::unique_ptr<Batch> &b, PairTurn &turn, Clock::time_point tp);
	void host_format_route(Worker &w, std::unique_ptr<Batch> &b, PairTurn &turn, Clock::time_point tp);
	bool gpu_bgzf_chunks(Worker &w, Batch &b); void recycle_input(Batch &b); void hand_to_writer(std::unique_ptr<Batch> &b, bool wait);
	// behind it
	void finish_sort(); void drain_side_outputs(); void report(double secs); void report_search_paths(); void teardown();
	template <class Finish, class Next> void drain(Finish finish, Next next, FILE *&file, const std::string &path, const char *tag, const std::function<void(const char *, size_t)> &tap = nullptr);

	// (every waiter looks at `failed`: wake them all -- ADVICE r3)
	void fail(const std::string &m2) {
		{ std::lock_guard<std::mutex> lk(fail_mu); if (!failed.exchange(true)) fail_msg = m2; }
		{ std::lock_guard<std::mutex> lk(out_mu); }
		out_cv.notify_all();
		{ std::lock_guard<std::mutex> lk(text_mu); }
		text_cv.notify_all();
	}
	std::string pipeline_error(long long rc, bool from_mapper = false) {   // (the sorter never spills: -12 from it, -28 through a mapper, ends the run with what it held)
		std::string e = ngm_pipeline_last_error();
		if (sorter && rc == (from_mapper ? -28 : -12)) {
			uint64_t sc[5] = {0, 0, 0, 0, 0};
			(void) ngm_bam_sort_stats(sorter, sc, nullptr);
			char pre[160];
			snprintf(pre, sizeof(pre), "--sort keeps the run's records in GPU memory (%.2f GiB so far): ", (double) sc[1] / (double) (1ull << 30));
			e = pre + e;
		}
		return e;
	}
	bool put_all(const char *p, size_t n, uint64_t off) {
		while (n) {
			// (4 MB pieces: 13.9 GB/s into the page cache against 9-11 GB/s for one call per 32 MB and more, profiles/r03_write_calibration.txt)
			const ssize_t w = pwrite(out_fd, p, std::min<size_t>(n, (size_t) 4 << 20), (off_t) off);
			if (w <= 0) return false;
			p += w; n -= (size_t) w; off += (uint64_t) w;
		}
		return true;
	}
	void strip_mate(const char *name, uint32_t &len) const {  // ReadProvider::NextRead (ReadProvider.cpp:419-422)
		if (len >= 2 && name[len - 2] == o.pe_delimiter) len -= 2;
	}
};

// --count: the BED file is read and checked against the contigs of the FASTA (names up to the first blank, 100 characters at most, contigs of
// 10 bases or fewer dropped: what refindex.cpp keeps) before any GPU work, so that a bad line costs no index build
// a side output's file is opened before the run, not after it
static FILE *open_before_run(const std::string &path) {
	FILE *f = fopen(path.c_str(), "wb");
	if (!f) die("cannot write " + path);
	return f;
}

void Run::read_count_regions() {
	if (o.count.empty()) return;
	gzFile f = gzopen(o.ref.c_str(), "rb");
	if (!f) die("--count: cannot open reference " + o.ref);
	std::string name;
	uint64_t len = 0;
	bool have = false, in_name = false, name_done = false, line_start = true;
	auto flush = [&]() { if (have && len > 10) { count_names.push_back(name.substr(0, 100)); count_lens.push_back((uint32_t) std::min<uint64_t>(len, 0xffffffffull)); } };
	std::vector<char> buf(1 << 20);
	int got;
	while ((got = gzread(f, buf.data(), (unsigned) buf.size())) > 0) {
		for (int i = 0; i < got; ++i) {
			const char ch = buf[i];
			if (ch == '\n') { line_start = true; in_name = false; continue; }
			if (line_start && ch == '>') { flush(); name.clear(); len = 0; have = true; in_name = true; name_done = false; line_start = false; continue; }
			line_start = false;
			if (in_name) { if (ch == ' ' || ch == '\t') name_done = true; else if (!name_done && ch != '\r') name.push_back(ch); }
			else if (have && ch != ' ' && ch != '\t' && ch != '\r') ++len;
		}
	}
	flush();
	gzclose(f);
	FILE *b = fopen(o.count.c_str(), "rb");
	if (!b) die("--count: cannot read " + o.count);
	std::string text;
	char chunk[65536];
	for (size_t k; (k = fread(chunk, 1, sizeof(chunk), b)) > 0;) text.append(chunk, k);
	fclose(b);
	std::vector<const char *> names;
	for (const std::string &n : count_names) names.push_back(n.c_str());
	std::string err;
	if (!ngm::cnt::parse_bed(text, (int) names.size(), names.data(), count_lens.data(), count_regions, &err)) die("--count: " + o.count + " " + err);
}

// SAM / BAM input (ReadProvider::DetermineParser): known from the first bytes, so that what it does not go with is refused before any GPU work
void Run::refuse_by_input_format() {
	for (const std::string *path : {&o.qry, &o.qry1, &o.qry2}) if (!path->empty()) in_format = std::max(in_format, (int) ngm::bamin::detect_file(path->c_str()));
	if (in_format == ngm::bamin::kFastx) return;
	const std::string what = in_format == ngm::bamin::kBam ? "BAM" : "SAM";
	info("INPUT", "Input is " + what);
	if (o.keep_tags) die("option --keep-tags is not supported by the HIP backend yet (" + what + " input: the tags of the input records are not copied to the output)");
	if (!o.qry1.empty() || !o.qry2.empty()) die(what + " input cannot be combined with --qry1/--qry2: give the interleaved mates to -p -q");
	if (o.broken_pairs) die(what + " input cannot be combined with --broken-pairs");
	if (o.shard_n > 1) die(what + " input cannot be combined with --shard");
	if (o.shard_output) die(what + " input cannot be combined with --shard-output");
	if (o.serial_reader) die(what + " input cannot be combined with --serial-reader: its records are read from the whole file in memory");
}

// a shard process of `-g a,b,... --shard-output` on distinct GPUs: join the communicator of the one collective of the path (the final
// statistics all-reduce, RCCL over xGMI) NOW, on a thread of its own -- ncclCommInitRank takes about a second, the load of the index hides it
void Run::join_communicator() {
	const char *id = getenv("NGM_HIP_RCCL_ID");
	if (!id || !(o.shard_n >= 1 && o.stats_fd >= 0)) return;
	const std::string id_s = id;
	stats_comm_thread = std::thread([this, id_s] {
		stats_comm = ngm_stats_comm_create(o.device, o.shard_i, o.shard_n, id_s.c_str());
		if (!stats_comm) stats_comm_error = ngm_pipeline_last_error();
	});
}

// Page-locked memory is requested NOW, by threads of its own, under the load of the index -- measured (4 M reads, MI355X box): requested
// after the sensitivity estimate it is 0.14 s on the input-to-output path, requested under the estimate it slows that estimate's driver
// calls from 0.04 to 0.14 s.  Its size depends on the longest read, which only the scan of the input knows: the first records give a
// guess, and take_pinned() asks again if the guess did not hold.
void Run::request_pinned_early() {
	if (!(route.gpu_sam || route.gpu_bgzf) || (o.qry.empty() && o.qry1.empty()) || o.out.empty()) return;
	size_t peek_max = 0;
	if (o.max_read_length > 0) peek_max = (size_t) o.max_read_length;
	else if (in_format == ngm::bamin::kFastx) {   // (SAM / BAM: no guess, the buffers are requested once the scan knows the longest read)
		SeqReader peek((o.qry1.empty() ? o.qry : o.qry1).c_str());
		Read r;
		for (int i = 0; i < 256 && peek.ok() && peek.next(r); ++i) if (!r.seq.empty()) peek_max = std::max(peek_max, ngm::trim::estimate_len(r.seq.size(), o.trim.trim5));
	}
	if (peek_max > 0) pinned.request(o.paired ? (o.batch & ~1) : o.batch, std::min(1000, (int) ((peek_max | 1) + 1)), route, o.devices.size() * (size_t) o.workers);
}

// an index cache next to the FASTA is loaded instead of rebuilding; a fresh build is saved for the next run unless
// --skip-save (src/PrefixTable.cpp:232-262, SequenceProvider.cpp:264-330)
void Run::load_reference() {
	const std::string ht_cache = o.ref + "-ht-" + std::to_string(o.kmer) + "-" + std::to_string(rp.kmer_skip) + ".3.ngm";
	ref = o.vcf.empty() ? ngm_ref_create_from_fasta(o.device, &rp, o.ref.c_str()) : ngm_ref_create_from_fasta_vcf(o.device, &rp, o.ref.c_str(), o.vcf.c_str());
	if (!ref) die(ngm_pipeline_last_error());
	const bool had_cache = ngm_ref_loaded_from_cache(ref) != 0;  // (an unreadable or corrupt cache was rebuilt and is rewritten below)
	if (had_cache) info("PREPROCESS", "Reading reference index from " + ht_cache);
	else if (!o.skip_save) {
		if (ngm_ref_write_ngm_cache(ref, o.ref.c_str()) < 0) info("PREPROCESS", std::string("could not save the index: ") + ngm_pipeline_last_error());
		else info("PREPROCESS", "Writing reference index to " + ht_cache);
	}
	if (!o.vcf.empty()) {
		uint64_t vs[6] = {0, 0, 0, 0, 0, 0}, sk[2] = {0, 0};
		if (ngm_ref_vcf_summary(ref, vs) == 1) {
			infof("PREPROCESS", "Loaded VCF (%llu variations)", (unsigned long long) vs[0]);
			infof("PREPROCESS", "Built SNP region table (%llu SNPs, %llu indels, %llu ignored)", (unsigned long long) vs[1], (unsigned long long) vs[2], (unsigned long long) vs[3]);
			// PrefixTable.cpp:439-443, its two arguments swapped as there
			if (ngm_ref_vcf_skip_counts(ref, sk) == 1 && sk[0] != sk[1]) {
				infof("PREPROCESS", "\tSkipBuild (%llu) != SkipCount (%llu)", (unsigned long long) sk[0], (unsigned long long) sk[1]);
			}
		} else if (had_cache) {
			info("PREPROCESS", "--vcf " + o.vcf + " not applied: the index is loaded from the existing cache " + ht_cache + " as it is (delete it to rebuild with the VCF)");
		}
	}
	// the layout the candidate search gathers from (canonical pair buckets) belongs to the preparation of the reference, not to the first batch
	if (ngm_ref_prepare_search(ref, o.bs_mapping) < 0) die(ngm_pipeline_last_error());
	info("PREPROCESS", "index entries: " + std::to_string(ngm_ref_index_entries(ref)) + ", max. k-mer frequency " +
			std::to_string(o.max_kfreq > 0 ? o.max_kfreq : ngm_ref_auto_max_kfreq(ref)));
	infof("PREPROCESS", "Reference and index ready: %.3f s (%s)", span_s(t_process), had_cache ? "loaded from the cache files" : "built");
}

// ---- pass 1: read lengths + the sample for the sensitivity estimate (ReadProvider.cpp:201-305); for a plain input also the record
// index the splitter cuts batches from.  Sets q, the corridor and the mapper parameters that do not depend on the estimate.
void Run::scan_input() {
	t_input = Clock::now();  // the first input byte is read below
	const bool interleaved = o.paired && !o.qry.empty();  // ReadProvider::GenerateRead (ReadProvider.cpp:526-584)
	path0 = o.paired ? (interleaved ? o.qry : o.qry1) : o.qry;
	path1 = (o.paired && !interleaved) ? o.qry2 : std::string();
	if (!o.serial_reader) {
		bool ok1 = true;
		std::thread second;   // (a .gz pair inflates both files at the same time)
		mf0.device = mf1.device = o.device;
		if (!path1.empty()) second = std::thread([&] { ok1 = mf1.open(path1.c_str()) && mf1.plain_fastq(); });
		plain = mf0.open(path0.c_str()) && (mf0.format != ngm::bamin::kFastx || mf0.plain_fastq());
		if (mf0.p && mf0.format != in_format) die("the input is not the " + std::string(in_format == ngm::bamin::kBam ? "BAM" : in_format == ngm::bamin::kSam ? "SAM" : "FASTA / FASTQ") + " file its first bytes announce");
		if (second.joinable()) second.join();
		plain = plain && ok1;
		if (!plain) { mf0.release(); mf1.release(); }   // (an inflated copy the serial reader has no use for)
	}
	if (in_format != ngm::bamin::kFastx && !plain) die("cannot read " + path0 + " into memory (SAM / BAM input is read from the whole file in memory)");
	batch_reads = o.paired ? (o.batch & ~1) : o.batch;
	// the splitter hands out whole sub-ranges of sub_step records (per file): the largest power of two up to kSub that divides a batch's share
	per_file_reads = path1.empty() ? batch_reads : batch_reads / 2;
	while (sub_step > 1 && per_file_reads % sub_step != 0) sub_step >>= 1;
	size_t max_len = 0, min_len = 9999999, sum_len = 0;
	// reads without a sequence are not counted (parseRead returns 0 for them: the `if (l > 0)` of ReadProvider.cpp:236)
	bool finish = false;
	auto account = [&](size_t seq_len) -> bool {  // true: keep this read for the sensitivity sample
		if (seq_len == 0) return false;
		const size_t len = ngm::trim::estimate_len(seq_len, o.trim.trim5);
		max_len = std::max(max_len, len); min_len = std::min(min_len, len); sum_len += len;
		++count;
		if (count % 1000 == 0 && count < 10000000) return true;
		if (count == 10000001) { if (o.argos || max_len - min_len >= 10) max_len = (size_t) (max_len * 1.1f); finish = true; }
		return false;
	};
	bool scan_finished = false;
	if (plain) {
		// both passes over a plain input are one parallel scan: record offsets for the splitter, lengths and the sample for the estimates
		mf0.prefault(); mf1.prefault();
		if (in_format != ngm::bamin::kFastx) {
			build_record_index(mf0, sub_step, o.trim.trim5, ix0);
			if (!ix0.ok) die(ix0.length_error);
		} else {
			build_fastq_index(mf0, sub_step, true, o.trim.trim5, ix0);
		}
		if (ix0.ok && mf1.p) build_fastq_index(mf1, sub_step, false, o.trim.trim5, ix1);
		if (!ix0.ok || (mf1.p && !ix1.ok)) {
			// not a strict 4-line record (multi-line sequences, stray blank lines): kseq reads those, so does the serial reader
			info("INPUT", "Record at byte " + std::to_string(!ix0.ok ? ix0.bad_at : ix1.bad_at) + " of " + (!ix0.ok ? path0 : path1) + " is not a 4-line FASTQ record: using the serial reader");
			plain = false; o.serial_reader = 1;
			mf0.release(); mf1.release();
		} else {
			const std::string &le = !ix0.length_error.empty() ? ix0.length_error : ix1.length_error;
			if (!le.empty()) die("Error while parsing read: sequence and quality lengths differ (" + le + ")");
			max_len = ix0.max_len; min_len = ix0.min_len; sum_len = ix0.sum_len; count = ix0.count;
			if (ix0.n_nonempty >= 10000001 && (o.argos || max_len - min_len >= 10)) max_len = (size_t) (max_len * 1.1f);
			scan_finished = ix0.n_nonempty >= 10000001;
			sample = std::move(ix0.sample);
		}
	}
	if (!plain) {
		SeqReader in(first_input.c_str());
		if (!in.ok()) die("cannot open " + first_input);
		Read r;
		while (!finish && in.next(r)) if (account(r.seq.size())) {
			if (o.trim.trim5 > 0) r.seq.erase(0, std::min<size_t>(r.seq.size(), (size_t) o.trim.trim5));
			sample.push_back(r);
		}
		scan_finished = finish;
	}
	// NGM.Stats->TotalSeqs (the --argos prolog): the reads the scan counted, 0 when it stopped at the 10 000 001st (ReadProvider.cpp:252-279)
	total_seqs = scan_finished ? 0 : count;
	if (count == 0) die("No reads found in input file.");
	if (o.max_read_length > 0) max_len = (size_t) o.max_read_length;
	q = (int) ((max_len | 1) + 1);
	avg_len = (int) (sum_len / count);
	if (q > 1000) q = 1000;
	const int corridor = o.corridor > 0 ? o.corridor : (int) (5 + avg_len * 0.15);
	infof("INPUT", "Average read length: %d (min: %zu, max: %d)", avg_len, min_len, q);
	info("INPUT", "Corridor width: " + std::to_string(corridor));

	mp.qry_max_len = q; mp.corridor = corridor; mp.match_bonus = o.match; mp.mismatch_penalty = o.mismatch;
	mp.gap_read_penalty = o.gap_read; mp.gap_ref_penalty = o.gap_ref; mp.mode = o.mode; mp.variant = o.variant;
	mp.sensitivity = 0.5f; mp.kmer_min = o.kmer_min; mp.max_cmrs = o.max_cmrs; mp.max_kfreq = o.max_kfreq;
	mp.hard_clip = o.hard_clip; mp.silent_clip = o.silent_clip;
	mp.personality = o.affine ? NGM_PERSONALITY_AFFINE : NGM_PERSONALITY_LINEAR; mp.gap_extend_penalty = o.gap_extend;
	mp.min_insert_size = o.min_insert; mp.max_insert_size = o.max_insert; mp.pair_score_cutoff = 0.9f;
	mp.topn = o.topn; mp.strata = o.strata;
	mp.bs_mapping = o.bs_mapping; mp.bs_cutoff = o.bs_cutoff; mp.bs_read_skip = o.kmer_skip; mp.match_bonus_tt = o.match_tt; mp.match_bonus_tc = o.match_tc; mp.slam_seq = o.slam_seq;
	if (o.paired) info("INPUT", "Input is paired end data.");
	t_indexed = Clock::now();
}

// (on its own thread the estimate never ends the process: its value is only logged there, so a failure is a note and the run goes on)
void Run::run_estimate(ngm_mapper_params ep, float &sens, bool &estimated, bool logged_only) {
	auto give_up = [&](const char *why) {
		if (!logged_only) die(why);
		info("INPUT", std::string("note: no sensitivity estimate (it is only logged with -s): ") + why);
	};
	ep.sensitivity = 0.0f;
	ep.slam_seq &= ~4;   // (the estimate looks the read k-mers up as they are: ReadProvider's own PrefixSearch, src/ReadProvider.cpp:79-124)
	const auto te0 = Clock::now();
	ngm_mapper *em = ngm_mapper_create(ref, &ep);
	if (!em) { give_up(ngm_pipeline_last_error()); return; }
	const auto te1 = Clock::now();
	const int ns = (int) sample.size();
	std::vector<char> rows((size_t) ns * q);
	for (int i = 0; i < ns; ++i) pack_row(sample[i], q, &rows[(size_t) i * q]);
	std::vector<uint32_t> offs(ns + 1);
	std::vector<float> mv(ns), both(ns);
	if (ngm_mapper_cs(em, ns, rows.data(), offs.data(), mv.data()) < 0 || ngm_mapper_cs_max_combined(em, both.data()) < 0) {
		const std::string why = ngm_pipeline_last_error();
		ngm_mapper_destroy(em);
		give_up(why.c_str());
		return;
	}
	float sum = 0.f;
	int n_used = 0;
	const int skip = o.kmer_skip + 1;
	for (int i = 0; i < ns; ++i) {
		const int L = (int) strnlen(&rows[(size_t) i * q], q);
		const int mx = (int) ceil((L - o.kmer + 1) / skip * 1.0);
		if (mx > 1.0f && both[i] <= mx) { sum += both[i] / mx; ++n_used; }
	}
	const auto te2 = Clock::now();
	ngm_mapper_destroy(em);
	if (getenv("NGM_HIP_HOST_TIMING")) {
		infof("INPUT", "Sensitivity estimate, s: mapper (+ search layout of the index) %.3f | candidate search of %d reads %.3f | mapper released %.3f",
				span_s(te0, te1), ns, span_s(te1, te2), span_s(te2));
	}
	// ReadProvider.cpp:324-352; with no usable sample read the average is 0/0 = NaN and std::max(0.3f, NaN) is 0.3
	const float avg = sum / n_used * 1.0f;
	sens = std::min(std::max(0.3f, avg), 0.9f);
	infof("INPUT", "Estimated sensitivity: %f", sens);
	float modifier = 0;
	if (o.very_fast) modifier = 0.7f * (1.0f - sens);
	else if (o.fast) modifier = 0.35f * (1.0f - sens);
	else if (o.very_sensitive) modifier = -0.7f * sens;
	else if (o.sensitive) modifier = -0.35f * sens;
	sens += modifier;
	estimated = true;
	// the reference hands the estimate to the search through its string-typed configuration: Override("sensitivity",
	// float) prints it with "%f" (src/config/Config.cpp:185-189) and CS reads it back with atof -- six decimals.  On a
	// threshold like 29 votes x 0.7241379 = 21 that rounding decides whether a 21-vote region is a candidate (found by
	// the drop-in run of the real program, tests/test_gpu_dropin.py)
	{ char b[32]; snprintf(b, sizeof(b), "%f", sens); sens = (float) atof(b); }
}

// ---- sensitivity (ReadProvider.cpp:310-385) -----------------------------------------------------------
// The estimate of the reference runs even when -s sets the value (its result is then only logged, ReadProvider.cpp:359-365): in that
// case it runs beside the set-up of the mappers instead of in front of it.
void Run::estimate_sensitivity() {
	float sens = 0.5f;
	bool estimated = false;
	if (o.bs_mapping) {
		if (o.sensitivity < 0) info("INPUT", "Sensitivity parameter set to 0.5");   // ReadProvider.cpp:317, :378-386: no estimate in this mode
		estimated = true;
	} else if (count >= 1000 && !sample.empty()) {
		if (o.sensitivity >= 0) estimate_thread = std::thread([this, ep = mp] { float s2 = 0.5f; bool e2 = false; run_estimate(ep, s2, e2, true); });
		else run_estimate(mp, sens, estimated, false);
	}
	if (o.sensitivity >= 0) sens = o.sensitivity;
	else if (!estimated) info("INPUT", "Sensitivity parameter neither set nor estimated. Falling back to default.");
	mp.sensitivity = sens;
	t_estimated = Clock::now();
}

// ---- output ------------------------------------------------------------------------------------------------------
// the output is written by the writer thread alone, in input order.  Measured alternatives (round 2, 10 M reads, 4.2 GB of
// SAM): pwrite from the pool threads -- the writes serialise on the file's inode lock and the threads queueing there are
// missing from the pool (3.5 M reads/s with 65 chunks per batch, 2.8 M and 32 s of system time with 500); a shared file
// mapping of each batch's range filled by the pool -- 1.6 M reads/s, the page faults cost more than the lock.
void Run::write_header() {
	out_fd = ::open(o.out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
	if (out_fd < 0) die("cannot write " + o.out);
	if (o.sort) (void) unlink((o.out + ".bai").c_str());   // (an index of an earlier file must not stand beside this one if the run fails)
	for (int i = 0; i < ngm_ref_contig_count(ref); ++i) { contig_names.push_back(ngm_ref_contig_name(ref, i)); contig_lens.push_back(ngm_ref_contig_len(ref, i)); }
	if (o.sort) for (size_t i = 0; i < contig_lens.size(); ++i) if (contig_lens[i] > ((uint64_t) 1 << 29))
		die("--sort cannot index contig " + contig_names[i] + ": it has more than 2^29 bases, beyond what a BAI index reaches (a CSI index is not built)");
	static const char *tag[12] = {"ID", "CN", "DS", "DT", "FO", "KS", "LB", "PG", "PI", "PL", "PU", "SM"};
	std::string h = o.sort ? "@HD\tVN:1.0\tSO:coordinate\n" : "@HD\tVN:1.0\tSO:unsorted\n";
	std::string rg;
	if (!o.rg[0].empty()) {  // SAMWriter.cpp:46-80
		rg = "@RG\tID:" + o.rg[0];
		for (int t = 1; t < 12; ++t) if (!o.rg[t].empty()) { rg += "\t"; rg += tag[t]; rg += ":" + o.rg[t]; }
		rg += "\n";
	}
	std::string z;   // what goes in front of the records
	bool with_every_shard = false;   // (--shard i/N: the header travels with the first shard)
	if (o.argos) {
		// ScoreWriter::DoWriteProlog (ScoreWriter.cpp:19-35)
		const int plen = ngm_argos_prolog(ref, total_seqs, nullptr, 0);
		if (plen < 0) die(ngm_pipeline_last_error());
		z.assign((size_t) plen, '\0');
		if (ngm_argos_prolog(ref, total_seqs, &z[0], z.size()) != plen) die(ngm_pipeline_last_error());
		with_every_shard = true;
	} else if (!o.bam) {
		for (size_t i = 0; i < contig_names.size(); ++i) { h += "@SQ\tSN:" + contig_names[i] + "\tLN:"; put_u64(h, contig_lens[i]); h += "\n"; }
		h += "@PG\tID:ngm\tPN:ngm\tVN:0.5.5-hip\tCL:\"" + o.cmdline + "\"\n";
		h += rg;
		z.swap(h);
	} else {
		// BAMWriter::DoWriteProlog (BAMWriter.cpp:18-110) through bamtools' SamFormatPrinter: @HD, @RG, @PG (ID PN CL VN); the
		// contigs only in the binary dictionary
		h += rg;
		h += "@PG\tID:ngm\tPN:ngm\tCL:\"" + o.cmdline + "\"\tVN:0.5.5-hip\n";
		std::string raw;
		ngm::bam::put_header(raw, h, contig_names, contig_lens);
		if (!ngm::bam::bgzf_compress(raw.data(), raw.size(), z)) die("BGZF compression failed");
	}
	if (with_every_shard || o.shard_i == 0) {
		if (!put_all(z.data(), z.size(), out_off)) die("write error on " + o.out);
		out_off += z.size();
	}
}

// ---- the references / mappers: one reference per GPU (the first one exists), `workers` mappers per GPU ---------------
void Run::create_mappers_and_side_outputs() {
	refs.assign(1, ref);
	for (size_t d = 1; d < o.devices.size(); ++d) {
		ngm_ref *r2 = ngm_ref_create_from_fasta(o.devices[d], &rp, o.ref.c_str());  // the cache written above loads in seconds
		if (!r2 || ngm_ref_prepare_search(r2, o.bs_mapping) < 0) die(ngm_pipeline_last_error());
		refs.push_back(r2);
	}
	pair_state = ngm_pair_state_create();
	workers = std::vector<Worker>(o.devices.size() * (size_t) o.workers);
	for (size_t w = 0; w < workers.size(); ++w) {
		workers[w].m = ngm_mapper_create(refs[w % refs.size()], &mp);
		if (!workers[w].m) die(ngm_pipeline_last_error());
		ngm_mapper_set_pair_state(workers[w].m, pair_state);
		ngm_mapper_set_fast_pairing(workers[w].m, o.fast_pairing);
		if (o.argos) {
			if (ngm_mapper_set_argos(workers[w].m, o.argos_min) < 0) die(ngm_pipeline_last_error());
		} else if (route.gpu_sam) {
			ngm_sam_options so{};
			so.paired = o.paired; so.min_insert_size = o.min_insert; so.max_insert_size = o.max_insert; so.min_mq = o.min_mq;
			so.min_identity = o.min_identity; so.min_residues = o.min_residues; so.no_unal = o.no_unal; so.rg_id = o.rg[0].empty() ? nullptr : o.rg[0].c_str(); so.bs_mapping = o.bs_mapping; so.slam_seq = o.slam_seq; so.bam = o.bam ? 1 : 0;
			if (ngm_mapper_set_sam_options(workers[w].m, &so) < 0) die(ngm_pipeline_last_error());
		}
		ngm_mapper_set_reference_cs_batch(workers[w].m, 1800000 / std::max(1, avg_len));
		ngm_mapper_set_reference_score_buffer(workers[w].m, o.ref_score_buffer);
		if (route.gpu_bgzf) {
			workers[w].bz = ngm_bgzf_create(o.devices[w % o.devices.size()]);
			if (!workers[w].bz) die(ngm_pipeline_last_error());
		}
	}
	// --sort, --coverage, --snp: one object each on the first device, held for the whole run.  The mappers of the GPU-text route feed them
	// (in place on that GPU, through the library's add calls from the others); the host-formatted routes through the formatter's callbacks
	if (o.sort) {
		ngm_bam_sort_params sp{};
		sp.device = o.devices[0];
		sorter = ngm_bam_sort_create(&sp);
		if (!sorter) die(ngm_pipeline_last_error());
		if (o.markdup && ngm_bam_sort_set_markdup(sorter, 1) < 0) die(ngm_pipeline_last_error());
		if (route.gpu_sam) for (Worker &w : workers) if (ngm_mapper_set_bam_sorter(w.m, sorter) < 0) die(ngm_pipeline_last_error());
	}
	uint64_t bases = 0;
	for (size_t i = 0; i < contig_lens.size(); ++i) bases += contig_lens[i];
	if (!o.coverage.empty()) {
		coverage_file = open_before_run(o.coverage);
		std::vector<uint32_t> lens32;
		std::vector<const char *> names;
		for (size_t i = 0; i < contig_lens.size(); ++i) { lens32.push_back((uint32_t) contig_lens[i]); names.push_back(contig_names[i].c_str()); }
		ngm_coverage_params cp{};
		cp.device = o.devices[0]; cp.n_ref = (int) lens32.size(); cp.ref_len = lens32.data(); cp.ref_name = names.data();
		coverage = ngm_coverage_create(&cp);
		if (!coverage) die(std::string("--coverage: ") + ngm_pipeline_last_error());
		infof("MAIN", "Coverage counters: %.1f MiB on GPU %d (4 bytes per base of the reference, held for the whole run)", (double) (bases + lens32.size()) * 4.0 / (double) (1 << 20), o.devices[0]);
		if (route.gpu_sam) for (Worker &w : workers) if (ngm_mapper_set_coverage(w.m, coverage) < 0) die(ngm_pipeline_last_error());
	}
	if (!o.snp.empty()) {   // coverage's counters and three mismatch counters per base, beside that GPU's resident reference
		snp_file = open_before_run(o.snp);
		ngm_snp_params sp{};
		sp.min_cov = (uint32_t) o.snp_min_cov; sp.min_frac = o.snp_min_frac; sp.min_qual = (int) o.snp_min_qual; sp.min_frac_text = o.snp_frac_text.c_str();
		snp = ngm_snp_create_for_ref(refs[0], &sp);
		if (!snp) die(std::string("--snp: ") + ngm_pipeline_last_error());
		infof("MAIN", "SNP counters: %.1f MiB on GPU %d (16 bytes per base of the reference, held for the whole run)", (double) (bases + contig_lens.size()) * 16.0 / (double) (1 << 20), o.devices[0]);
		if (route.gpu_sam) for (Worker &w : workers) if (ngm_mapper_set_snp(w.m, snp) < 0) die(ngm_pipeline_last_error());
	}
	if (!o.count.empty()) {   // two counters per base of the union of the regions and two per region, beside that GPU's resident reference
		// (the regions were checked against the FASTA's contigs: they must be the reference's, whether it was built or loaded from its cache)
		bool same = count_names.size() == contig_names.size();
		for (size_t i = 0; same && i < contig_names.size(); ++i) same = count_names[i] == contig_names[i] && count_lens[i] == contig_lens[i];
		if (!same) die("--count: the contigs read from " + o.ref + " for the BED file (" + std::to_string(count_names.size()) + ") are not the reference's (" + std::to_string(contig_names.size()) +
				"): either the index cache next to it was built from another FASTA (delete it to rebuild it), or the file has a form the two readers take differently");
		count_file = open_before_run(o.count_out);
		std::vector<int32_t> r_ref;
		std::vector<uint32_t> r_start, r_end;
		std::string r_strand;
		for (const ngm::cnt::Region &r : count_regions) { r_ref.push_back(r.contig); r_start.push_back(r.start); r_end.push_back(r.end); r_strand.push_back(r.strand); }
		ngm_count_params cp{};
		cp.min_qual = (int) o.count_min_qual; cp.n_regions = count_regions.size(); cp.region_ref = r_ref.data(); cp.region_start = r_start.data(); cp.region_end = r_end.data(); cp.region_strand = r_strand.data();
		counter = ngm_count_create_for_ref(refs[0], &cp);
		if (!counter) die(std::string("--count: ") + ngm_pipeline_last_error());
		ngm::cnt::Tables tab;
		tab.build(count_regions, (int) contig_names.size());
		infof("MAIN", "Conversion counters: %zu regions over %llu bases, %.1f MiB on GPU %d (8 bytes per base of the regions' union, held for the whole run)", count_regions.size(),
				(unsigned long long) tab.slots, (double) tab.slots * 8.0 / (double) (1 << 20), o.devices[0]);
		if (route.gpu_sam) for (Worker &w : workers) if (ngm_mapper_set_count(w.m, counter) < 0) die(ngm_pipeline_last_error());
	}
	if (!o.methyl.empty()) {   // a pair of counters (meth, unmeth) per base, beside that GPU's resident reference
		methyl_file = open_before_run(o.methyl);
		ngm_methyl_params mp{};
		mp.min_qual = (int) o.methyl_min_qual; mp.min_depth = (int) o.methyl_min_depth; mp.context = o.methyl_context.c_str();
		methyl = ngm_methyl_create_for_ref(refs[0], &mp);
		if (!methyl) die(std::string("--methyl: ") + ngm_pipeline_last_error());
		infof("MAIN", "Methylation counters: %.1f MiB on GPU %d (8 bytes per base of the reference, held for the whole run)", (double) bases * 8.0 / (double) (1 << 20), o.devices[0]);
		if (route.gpu_sam) for (Worker &w : workers) if (ngm_mapper_set_methyl(w.m, methyl) < 0) die(ngm_pipeline_last_error());
	}
}

// the host formatter (cli_format.h), built once from plain values
void Run::setup_formatter() {
	fmt.min_identity = o.min_identity; fmt.min_residues = o.min_residues; fmt.min_mq = o.min_mq;
	fmt.paired = o.paired; fmt.topn = route.topn; fmt.strata = o.strata; fmt.bam = o.bam; fmt.clip = o.hard_clip || o.silent_clip; fmt.no_unal = o.no_unal;
	fmt.bs_mapping = o.bs_mapping; fmt.slam_seq = o.slam_seq; fmt.variant = o.variant; fmt.xa_tag = o.trim.max_polya >= 0;
	fmt.set_read_group(o.rg[0]);
	fmt.contig_names = contig_names;
	fmt.q = q; fmt.stride = (size_t) 4 * q;
	fmt.min_insert = o.min_insert; fmt.max_insert = o.max_insert > 0 ? o.max_insert : 2147483647;
	fmt.ref_classes = [this](int contig, uint64_t pos, int span, uint8_t *out) { (void) ngm_ref_host_classes(ref, ngm_ref_contig_start(ref, contig) + pos, span, out); };
	if (coverage) fmt.add_coverage = [this](const CovAcc &a) { if (ngm_coverage_add(coverage, a.ref.data(), a.pos.data(), a.off.data(), a.text.data(), a.ref.size()) < 0) cov_failed = true; };
	if (snp) fmt.add_snp = [this](const SnpAcc &a, bool has_qual) {
		if (ngm_snp_add(snp, a.ref.data(), a.pos.data(), a.off.data(), a.text.data(), a.seq_off.data(), a.seq.data(), has_qual ? a.qual.c_str() : nullptr, a.ref.size()) < 0) snp_failed = true;
	};
	if (counter) fmt.add_count = [this](const SnpAcc &a, bool has_qual) {
		if (ngm_count_add(counter, a.ref.data(), a.pos.data(), a.off.data(), a.text.data(), a.seq_off.data(), a.seq.data(), has_qual ? a.qual.c_str() : nullptr, a.rev.data(), a.ref.size()) < 0) count_failed = true;
	};
	if (methyl) fmt.add_methyl = [this](const MethylAcc &a, bool has_qual) {
		if (ngm_methyl_add(methyl, a.ref.data(), a.pos.data(), a.off.data(), a.text.data(), a.seq_off.data(), a.seq.data(), has_qual ? a.qual.c_str() : nullptr, a.bottom.data(), a.ref.size()) < 0) methyl_failed = true;
	};
}

// ---- the splitter: plain input ---------------------------------------------------------------------------------------------
// record boundaries: the index of the estimation pass (every sub_step-th record offset per file, so that a batch is parsed in parallel)
void Run::split_plain() {
	uint64_t seq = 0;
	const bool two = !path1.empty();
	const char *uneven = "Error in input file. Number of reads in input not even. Please check the input or mapped in single-end mode.";
	if (two ? ix0.n_records != ix1.n_records : (o.paired && (ix0.n_records & 1))) fail(uneven);
	auto take = [&](const FastqIndex &ix, size_t r0, int cnt, std::vector<size_t> &sub) {
		const size_t s0 = r0 / (size_t) sub_step, s1 = (r0 + (size_t) cnt + (size_t) sub_step - 1) / (size_t) sub_step;
		sub.assign(ix.sub.begin() + (long) s0, ix.sub.begin() + (long) s1 + 1);
	};
	// --shard i/N: records [lo, hi) of each file, the boundaries on whole sub-ranges (and whole pairs of an interleaved file)
	const size_t gran = (size_t) std::max(sub_step, (o.paired && !two) ? 2 : 1);
	auto bound = [&](int i) -> size_t { return i >= o.shard_n ? ix0.n_records : (size_t) ((unsigned __int128) ix0.n_records * (unsigned) i / (unsigned) o.shard_n) / gran * gran; };
	const size_t rec_lo = bound(o.shard_i), rec_hi = bound(o.shard_i + 1);
	// (a quarter-size first batch per worker, so that the writer starts earlier, was measured slower: mapping pass 0.57 / 0.64 s against 0.52 / 0.54 s)
	const int first_div = 1;
	const size_t first_share = std::max<size_t>((size_t) sub_step, (size_t) per_file_reads / (size_t) first_div / (size_t) sub_step * (size_t) sub_step);
	for (size_t r0 = rec_lo, step = 0; !failed && r0 < rec_hi; r0 += step) {
		auto b = std::make_unique<Batch>();
		step = seq < workers.size() ? first_share : (size_t) per_file_reads;
		b->seq = seq++;
		b->n0 = (int) std::min<size_t>(step, rec_hi - r0);
		take(ix0, r0, b->n0, b->sub0);
		if (two) { b->n1 = b->n0; take(ix1, r0, b->n1, b->sub1); }
		b->n = b->n0 + b->n1;
		q_in->push(std::move(b));
	}
}

// ---- ... and the serial kseq-style reader (gz too large to inflate into memory, FASTA, multi-line records, --broken-pairs) -----------
void Run::split_serial() {
	uint64_t seq = 0;
	SeqReader in1(path0.c_str());
	std::unique_ptr<SeqReader> in2(path1.empty() ? nullptr : new SeqReader(path1.c_str()));
	if (!in1.ok() || (in2 && !in2->ok())) { fail(o.paired ? "cannot open the paired-end input" : "cannot open " + path0); return; }
	auto b = std::make_unique<Batch>();
	Read a, c, spare;
	bool have_spare = false;
	const uint64_t bp_units_per_batch = std::max<uint64_t>(1, (uint64_t) ((1800000 / std::max(1, avg_len)) & ~1) / 2);   // CS.cpp:26, :542; NGM.cpp:237-242
	uint64_t bp_units = 0, bp_reads = 0, bp_cur_start = 0;
	for (;;) {
		if (failed) break;
		if (!o.paired) {
			if (!in1.next(a)) break;
			b->owned.push_back(std::move(a));
		} else if (o.broken_pairs) {
			// ReadProvider::GenerateRead with acceptBrokenPaired (ReadProvider.cpp:529-575): two consecutive records whose names differ are
			// not mates -- the first is mapped alone (its mate's row holds a placeholder), the second becomes the first of the next pair;
			// a record left over at the end is mapped alone too.  Read ids (NGM.cpp:252-267): a batch of the reference's CS thread hands out
			// ids m_CurStart + 2 j, + 1 to its j-th pair and then advances m_CurStart by the reads it actually got -- after an odd number
			// the first mates of the following batch carry ODD ids, and SAMWriter::DoWritePair (SAMWriter.cpp:235-244) gives them 0x80
			if (have_spare) { a = std::move(spare); have_spare = false; }
			else if (!in1.next(a)) break;
			const bool hb = in1.next(c);
			uint32_t la = (uint32_t) a.name.size(), lc = (uint32_t) c.name.size();
			strip_mate(a.name.data(), la);
			if (hb) strip_mate(c.name.data(), lc);
			const bool mates = hb && la == lc && memcmp(a.name.data(), c.name.data(), la) == 0;
			const uint8_t swp = (bp_cur_start & 1) ? 4 : 0;
			if (mates) { a.unit = swp; c.unit = swp; b->owned.push_back(std::move(a)); b->owned.push_back(std::move(c)); bp_reads += 2; }
			else {
				a.unit = 1;
				b->owned.push_back(std::move(a));
				Read ph; ph.unit = 2;
				b->owned.push_back(std::move(ph));
				bp_reads += 1;
				if (hb) { spare = std::move(c); have_spare = true; }
			}
			if (++bp_units == bp_units_per_batch) { bp_cur_start += bp_reads; bp_units = 0; bp_reads = 0; }
		} else {
			const bool ha = in1.next(a), hb = ha ? (in2 ? in2->next(c) : in1.next(c)) : false;
			if (!ha) break;
			if (!hb) { fail("Error in input file. Number of reads in input not even. Please check the input or mapped in single-end mode."); break; }
			b->owned.push_back(std::move(a)); b->owned.push_back(std::move(c));
		}
		if ((int) b->owned.size() >= batch_reads) { b->seq = seq++; b->n = (int) b->owned.size(); q_in->push(std::move(b)); b = std::make_unique<Batch>(); }
	}
	if (!failed && !b->owned.empty()) { b->seq = seq++; b->n = (int) b->owned.size(); q_in->push(std::move(b)); }
}

void Run::splitter_main() {
	if (plain) split_plain();
	else if (o.shard_n > 1) fail("--shard needs 4-line FASTQ input (plain, or .gz small enough to be inflated into memory): the shard boundaries come from the record index");
	else split_serial();
	q_in->close();
}

// The page-locked buffers of the workers and the text pool: those requested under the index load if the guess of q held, else -- GPU-text
// route only; the buffers of the GPU BGZF route carry their sizes, a batch that needs more replaces them -- requested again, at once
// (measured: requesting them under the sensitivity estimate slows the driver calls of that estimate down by more than it saves)
void Run::take_pinned() {
	text_cap0 = (size_t) batch_reads * ((size_t) 2 * q + 288) + (1u << 20);
	pinned.join();
	if (pinned.bam && route.gpu_bgzf && pinned.w.size() == workers.size()) {
		for (size_t i = 0; i < workers.size(); ++i) if (pinned.w[i].bam_raw && pinned.w[i].bam_out) {
			workers[i].bam_raw = pinned.w[i].bam_raw; workers[i].bam_out = pinned.w[i].bam_out;
			workers[i].bam_raw_cap = pinned.bam_raw_cap; workers[i].bam_out_cap = pinned.bam_out_cap;
			pinned.w[i].bam_raw = pinned.w[i].bam_out = nullptr;
		}
	}
	const bool guess_held = route.gpu_sam && pinned.q >= q && pinned.batch == batch_reads && pinned.w.size() == workers.size() && pinned.complete();
	if (!guess_held) pinned.release();
	if (!route.gpu_sam) return;
	if (!guess_held) {
		pinned.request(batch_reads, q, route, workers.size());
		pinned.join();
		if (!pinned.complete()) die(ngm_pipeline_last_error());
	}
	text_free = pinned.text;
	for (size_t i = 0; i < workers.size(); ++i) {
		Worker &w = workers[i];
		w.rows = pinned.w[i].rows; w.qrows = pinned.w[i].qrows; w.meta = pinned.w[i].meta; w.names = pinned.w[i].names;
		w.rows_cap = (size_t) batch_reads * pinned.q; w.names_cap = (size_t) batch_reads * 32;
	}
	pinned.text.clear(); pinned.w.clear();
}

// ---- the worker: parse ------------------------------------------------------------------------------------------------------
// the batch's records as views (b.recs) and as rows in the worker's page-locked buffer, by the pool; false: the run has failed
bool Run::parse_batch(Worker &w, Batch &b) {
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	const int n = b.n;
	if ((size_t) n * q > w.rows_cap) {
		ngm_host_free(w.rows);
		w.rows_cap = (size_t) std::max(n, batch_reads) * q;
		w.rows = (char *) ngm_host_alloc(w.rows_cap);
		if (!w.rows) { fail(ngm_pipeline_last_error()); w.rows_cap = 0; }
		if (route.gpu_sam && w.rows) {
			ngm_host_free(w.qrows); ngm_host_free(w.meta);
			w.qrows = (char *) ngm_host_alloc(w.rows_cap);
			w.meta = (ngm_sam_read *) ngm_host_alloc((size_t) std::max(n, batch_reads) * sizeof(ngm_sam_read));
			if (!w.qrows || !w.meta) { fail(ngm_pipeline_last_error()); ngm_host_free(w.rows); w.rows = nullptr; w.rows_cap = 0; }
		}
	}
	{
		std::lock_guard<std::mutex> lk(spare_mu);
		if (!spare_recs.empty()) { b.recs = std::move(spare_recs.back()); spare_recs.pop_back(); }
		if (!spare_chunks.empty()) { b.chunks = std::move(spare_chunks.back()); spare_chunks.pop_back(); }
	}
	b.recs.resize(n);
	std::atomic<bool> bad{false};
	std::string bad_msg;
	// the end of every record's parse: the mate suffix off its name, -5 / --max-polya, its row; its qualities' row for the GPU writers
	auto finish_rec = [&](Rec &r, int i) {
		if (o.paired) strip_mate(r.name, r.name_len);
		r.polya = (uint16_t) ngm::trim::parse_read(o.trim, q, r.seq, r.seq_len, r.qual, r.qual_len, w.rows + (size_t) i * q);
		if (route.gpu_sam) memcpy(w.qrows + (size_t) i * q, r.qual, std::min<size_t>(r.qual_len, (size_t) q - 1));
	};
	if (w.rows && !b.owned.empty()) {
		pool.parallel_for(n, [&](int lo, int hi) {
			for (int i = lo; i < hi; ++i) {
				const Read &r = b.owned[i];
				b.recs[i] = Rec{r.name.data(), r.seq.data(), r.qual.data(), (uint32_t) r.name.size(), (uint32_t) r.seq.size(), (uint32_t) r.qual.size(), r.unit, 0};
				finish_rec(b.recs[i], i);
			}
		}, 4096);
	} else if (w.rows && in_format != ngm::bamin::kFastx) {
		// SAM / BAM input: the sub-ranges of the plain route; a record's views point into the file or into the sub-range's store
		namespace bi = ngm::bamin;
		const int nsub0 = (int) b.sub0.size() - 1;
		b.store.clear(); b.store.resize((size_t) nsub0);
		pool.parallel_for(nsub0, [&](int lo, int hi) {
			for (int sl = lo; sl < hi; ++sl) {
				const int cnt = std::min(sub_step, b.n0 - sl * sub_step);
				size_t at = b.sub0[sl];
				b.store[sl].reset(new char[2 * (b.sub0[sl + 1] - at) + 16]);
				char *store = b.store[sl].get();
				for (int j = 0; j < cnt; ++j) {
					const int i = sl * sub_step + j;
					bi::View v;
					if (in_format == bi::kBam) {
						size_t size = 0;
						uint32_t ls = 0;
						std::string err;
						if (!bi::bam_check((const uint8_t *) mf0.p, mf0.n, at, &size, &ls, &err)) { if (!bad.exchange(true)) bad_msg = err; return; }
						bi::bam_decode((const uint8_t *) mf0.p, at, v, store);
						store += bi::bam_store_bytes(ls);
						at += size;
					} else {
						size_t next = at;
						while (at < mf0.n && !bi::sam_is_record(mf0.p, mf0.n, at, &next)) at = next;
						if (at >= mf0.n || !bi::sam_decode(mf0.p, at, next, v, store)) { if (!bad.exchange(true)) bad_msg = "malformed SAM record at byte " + std::to_string(at); return; }
						store += bi::sam_store_bytes(at, next);
						at = next;
					}
					b.recs[i] = Rec{v.name, v.seq, v.qual, v.name_len, v.seq_len, v.qual_len, 0, 0};
					finish_rec(b.recs[i], i);
				}
			}
		}, 1);
	} else if (w.rows) {
		// plain input: sub-range s of file f holds records [s sub_step, ...) of that file's share of the batch; record j of file f is batch record
		// j (one file) or 2 j + f (two files)
		const bool two = b.n1 > 0;
		const int nsub0 = (int) b.sub0.size() - 1, nsub1 = two ? (int) b.sub1.size() - 1 : 0;
		pool.parallel_for(nsub0 + nsub1, [&](int lo, int hi) {
			CpuTime acc{t_parse_cpu_us};
			for (int sidx = lo; sidx < hi; ++sidx) {
				const int f = sidx < nsub0 ? 0 : 1, sl = f ? sidx - nsub0 : sidx;
				const MappedFile &mf = f ? mf1 : mf0;
				const std::vector<size_t> &sub = f ? b.sub1 : b.sub0;
				const int cnt = std::min(sub_step, (f ? b.n1 : b.n0) - sl * sub_step);
				size_t at = sub[sl];
				for (int j = 0; j < cnt; ++j) {
					const int i = two ? 2 * (sl * sub_step + j) + f : sl * sub_step + j;
					Rec &r = b.recs[i];
					const size_t nx = mf.record(at, r);
					if (!nx) { if (!bad.exchange(true)) bad_msg = "malformed FASTQ record at byte " + std::to_string(at); return; }
					if (r.qual_len != r.seq_len) { if (!bad.exchange(true)) bad_msg = "Error while parsing read: sequence and quality lengths differ (" + std::string(r.name, r.name_len) + ")"; return; }  // IParser.h copyToRead
					at = nx;
					finish_rec(r, i);
				}
			}
		}, 1);
	}
	if (bad) fail(bad_msg);
	return !failed;
}

// mates carry the same name (ReadProvider.cpp:540-575): the first pair of the batch that does not ends the run
void Run::check_mate_names(const Batch &b) {
	const int n = b.n;
	std::atomic<int> first_bad{n};
	ngm::ThreadPool::instance().parallel_for(n / 2, [&](int lo, int hi) {
		for (int pi = lo; pi < hi; ++pi) {
			const Rec &a = b.recs[2 * pi], &c = b.recs[2 * pi + 1];
			if (c.unit & 2) continue;   // --broken-pairs: a read without its mate
			if (a.name_len != c.name_len || memcmp(a.name, c.name, a.name_len) != 0) {
				int seen = first_bad.load();
				while (2 * pi < seen && !first_bad.compare_exchange_weak(seen, 2 * pi)) {}
				return;
			}
		}
	}, 8192);
	if (first_bad.load() < n) {
		const Rec &a = b.recs[first_bad.load()], &c = b.recs[first_bad.load() + 1];
		fail("Error while reading paired end reads. Names of mates don't match: " + std::string(a.name, a.name_len) + " and " + std::string(c.name, c.name_len) + ".");
	}
}

// a formatted batch is done with its record views and with the records of the serial reader
void Run::recycle_input(Batch &b) {
	{ std::lock_guard<std::mutex> lk(spare_mu); b.recs.clear(); spare_recs.push_back(std::move(b.recs)); }
	b.owned.clear(); b.owned.shrink_to_fit();
}

// ... and goes to the writer.  wait: back-pressure -- formatted batches wait here while the writer is behind, except the one it is waiting for
// (the GPU-text route is bounded by its text buffers instead)
void Run::hand_to_writer(std::unique_ptr<Batch> &b, bool wait) {
	{
		std::unique_lock<std::mutex> lk(out_mu);
		if (wait) out_cv.wait(lk, [&] { return out_ready.size() < workers.size() + 2 || b->seq == next_write.load() || failed.load(); });
		out_ready[b->seq] = std::move(b);
	}
	out_cv.notify_all();
}

// ---- the worker: the GPU writes the batch's text (SAM lines, BAM records with their BGZF blocks, argos lines) ---------------------
void Run::gpu_text_route(Worker &w, std::unique_ptr<Batch> &b, PairTurn &turn, Clock::time_point tp) {
	const int n = b->n;
	const bool xa_tag = fmt.xa_tag;
	// names: one block of bytes per batch (offsets by a prefix sum over the records), plus what the record printer needs per read
	size_t total = 0;
	for (int i = 0; i < n; ++i) {
		const Rec &r = b->recs[i];
		w.meta[i].name_off = (uint32_t) total; w.meta[i].name_len = (uint16_t) std::min<uint32_t>(r.name_len, 65535u);
		w.meta[i].qual_len = (uint16_t) (std::min<uint32_t>(r.qual_len, 0x7FFFu) | (r.seq_len == 0 ? 0x8000u : 0u));
		total += w.meta[i].name_len;
	}
	if (total + 16 > w.names_cap) {
		ngm_host_free(w.names);
		w.names_cap = std::max(total + 16, (size_t) batch_reads * 32);
		w.names = (char *) ngm_host_alloc(w.names_cap);
		if (!w.names) { fail(ngm_pipeline_last_error()); w.names_cap = 0; return; }
	}
	if (xa_tag && (size_t) n > w.polya_cap) {
		ngm_host_free(w.polya);
		w.polya_cap = (size_t) std::max(n, batch_reads);
		w.polya = (uint16_t *) ngm_host_alloc(w.polya_cap * sizeof(uint16_t));
		if (!w.polya) { fail(ngm_pipeline_last_error()); w.polya_cap = 0; return; }
	}
	uint16_t *const polya = xa_tag ? w.polya : nullptr;
	ngm::ThreadPool::instance().parallel_for(n, [&](int lo, int hi) {
		for (int i = lo; i < hi; ++i) { memcpy(w.names + w.meta[i].name_off, b->recs[i].name, w.meta[i].name_len); if (polya) polya[i] = b->recs[i].polya; }
	}, 8192);
	t_parse_us += us_since(tp);
	auto tm = Clock::now();
	TextBuf tb{nullptr, 0};
	{
		// (buffers go out in no particular order and come back only when the writer has written batch `next_write`; the
		// worker that holds exactly that batch must never wait for one -- it takes a fresh buffer instead -- and nobody waits
		// once the run has failed)
		std::unique_lock<std::mutex> lk(text_mu);
		text_cv.wait(lk, [&] { return !text_free.empty() || b->seq == next_write.load() || failed.load(); });
		if (!text_free.empty()) { tb = text_free.back(); text_free.pop_back(); }
	}
	if (failed) { if (tb.p) { std::lock_guard<std::mutex> lk(text_mu); text_free.push_back(tb); } return; }
	if (!tb.p) {
		tb.cap = text_cap0;
		tb.p = (char *) ngm_host_alloc(tb.cap);
		if (!tb.p) { fail(ngm_pipeline_last_error()); return; }
	}
	uint64_t st[3] = {0, 0, 0};
	float sam_ms = 0.f;
	long long len = o.argos ? ngm_mapper_map_argos(w.m, n, w.rows, w.names, total, w.meta, tb.p, tb.cap, st, &sam_ms)
	                        : ngm_mapper_map_sam_trimmed(w.m, n, w.rows, w.qrows, w.names, total, w.meta, polya, tb.p, tb.cap, st, &sam_ms);
	turn.armed = false;   // (the map call has taken the turn, whatever it returned)
	if (len > (long long) tb.cap) {  // (long CIGAR / MD strings: a larger buffer for this batch)
		ngm_host_free(tb.p);
		tb.cap = (size_t) len + (1u << 20);
		tb.p = (char *) ngm_host_alloc(tb.cap);
		const int got = tb.p ? ngm_mapper_sam_fetch(w.m, tb.p, tb.cap) : -1;
		if (got < 0) len = got; else if (o.bam) len = got;   // (BAM: the BGZF blocks are made by the fetch; it says how long they are)
	}
	if (len < 0) { fail(pipeline_error(len, true)); std::lock_guard<std::mutex> lk(text_mu); if (tb.p) text_free.push_back(tb); text_cv.notify_one(); return; }
	t_map_us += us_since(tm);
	if (o.paired) { uint64_t ps3[3] = {0, 0, 0}; if (ngm_mapper_last_pair_stats(w.m, ps3) == 0) for (int k2 = 0; k2 < 3; ++k2) pair_stat[k2] += ps3[k2]; }
	{ float kms[8] = {0}; if (ngm_mapper_last_kernel_ms(w.m, kms) == 0) { double sum = sam_ms; for (int k2 = 0; k2 < 7; ++k2) sum += kms[k2]; t_gpu_us += (long long) (sum * 1000.0); } }
	t_sam_gpu_us += (long long) (sam_ms * 1000.0);
	b->text = tb.p; b->text_cap = tb.cap; b->text_len = (size_t) len;
	b->n_total = st[0]; b->n_mapped = st[1]; b->n_written = st[2];
	recycle_input(*b);
	hand_to_writer(b, false);
}

// ---- the worker: the GPU maps, the pool formats the records (cli_format.h), in chunks of whole pairs -----------------------------
void Run::host_format_route(Worker &w, std::unique_ptr<Batch> &b, PairTurn &turn, Clock::time_point tp) {
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	const int n = b->n, topn = route.topn;
	const size_t stride = fmt.stride;
	t_parse_us += us_since(tp);
	auto tm = Clock::now();
	w.hits.resize((size_t) n * topn); w.cig.resize((size_t) n * topn * stride); w.md.resize((size_t) n * topn * stride);
	const int rc = o.paired ? ngm_mapper_map_pe(w.m, n, w.rows, w.hits.data(), w.cig.data(), w.md.data())
	                        : ngm_mapper_map_se(w.m, n, w.rows, w.hits.data(), w.cig.data(), w.md.data());
	turn.armed = false;   // (the map call has taken the turn, whatever it returned)
	if (rc < 0) { fail(ngm_pipeline_last_error()); return; }
	t_map_us += us_since(tm);
	{ float kms[8] = {0}; if (ngm_mapper_last_kernel_ms(w.m, kms) == 0) { double sum = 0; for (int k2 = 0; k2 < 7; ++k2) sum += kms[k2]; t_gpu_us += (long long) (sum * 1000.0); } }
	auto tf = Clock::now();
	const int units = o.paired ? n / 2 : n, per = o.paired ? 2 : 1;
	const int n_chunks = std::max(1, std::min(units / 256 + 1, pool.size() * 8));  // many more chunks than threads: the slowest thread decides when the batch is done
	b->chunks.resize(n_chunks);
	for (std::string &c : b->chunks) c.clear();  // (keeps the capacity of the batch this vector served before)
	std::vector<HostFormatter::Counts> cc(n_chunks);
	const HostFormatter::Input in{b->recs.data(), w.hits.data(), w.rows, w.cig.data(), w.md.data()};
	pool.parallel_for(n_chunks, [&](int lo, int hi) {
		CpuTime acc{t_format_cpu_us};
		for (int c = lo; c < hi; ++c) {
			const int u0 = (int) ((long long) units * c / n_chunks), u1 = (int) ((long long) units * (c + 1) / n_chunks);
			HostFormatter::Counts loc;  // (not cc[c] directly: neighbouring chunks share cache lines, and these are bumped per record)
			fmt.format_range(in, u0 * per, u1 * per, b->chunks[c], loc);
			cc[c] = loc;
			if (o.bam && !route.gpu_bgzf && !b->chunks[c].empty()) {  // every chunk becomes whole BGZF blocks: they concatenate into one valid file
				std::string z;
				z.reserve(b->chunks[c].size() / 3 + 64);
				if (!ngm::bam::bgzf_compress(b->chunks[c].data(), b->chunks[c].size(), z)) fail("BGZF compression failed");
				b->chunks[c].swap(z);
			}
		}
	}, 1, (o.bam && !route.gpu_bgzf) ? ngm::ThreadPool::cpu_quota() : 0);   // (BAM with zlib: records + deflate keep every thread busy for the whole batch)
	for (const HostFormatter::Counts &c : cc) {
		b->n_total += c.total; b->n_mapped += c.mapped; b->n_written += c.written;
		for (int k = 0; k < 3; ++k) if (c.pair[k]) pair_stat[k] += c.pair[k];
	}
	auto add_failed = [&](const std::atomic<bool> &flag, const char *option) { if (flag) fail(std::string(option) + ngm_pipeline_last_error()); return (bool) flag; };
	if (add_failed(cov_failed, "--coverage: ") || add_failed(snp_failed, "--snp: ") || add_failed(count_failed, "--count: ") || add_failed(methyl_failed, "--methyl: ")) return;
	if (route.gpu_bgzf && !gpu_bgzf_chunks(w, *b)) return;
	recycle_input(*b);
	t_format_us += us_since(tf);
	hand_to_writer(b, true);
}

// the batch's records, chunk after chunk, in page-locked memory -> whole BGZF blocks from the GPU (a batch ends with a short
// block: batches -- and shards -- concatenate into one valid file) -> pieces for the writer.  false: the run has failed
bool Run::gpu_bgzf_chunks(Worker &w, Batch &b) {
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	const auto tz = Clock::now();
	const int n_chunks = (int) b.chunks.size();
	std::vector<size_t> off(n_chunks + 1, 0);
	for (int c = 0; c < n_chunks; ++c) off[c + 1] = off[c] + b.chunks[c].size();
	const size_t total = off[n_chunks];
	long long zlen = 0;
	if (total > 0) {
		if (total > w.bam_raw_cap) {
			ngm_host_free(w.bam_raw); ngm_host_free(w.bam_out);
			w.bam_raw_cap = total + total / 4 + (1u << 20); w.bam_out_cap = ngm_bgzf_bound(w.bam_raw_cap);
			w.bam_raw = (char *) ngm_host_alloc(w.bam_raw_cap); w.bam_out = (char *) ngm_host_alloc(w.bam_out_cap);
			if (!w.bam_raw || !w.bam_out) { w.bam_raw_cap = w.bam_out_cap = 0; fail(ngm_pipeline_last_error()); return false; }
		}
		pool.parallel_for(n_chunks, [&](int lo, int hi) { for (int c = lo; c < hi; ++c) memcpy(w.bam_raw + off[c], b.chunks[c].data(), b.chunks[c].size()); }, 1);
		if (sorter) {   // --sort: the batch's records go to the sorter as they are; the writer gets nothing now
			if (const int rc = ngm_bam_sort_add(sorter, b.seq, w.bam_raw, total); rc < 0) { fail(pipeline_error(rc)); return false; }
		} else {
			zlen = ngm_bgzf_compress(w.bz, w.bam_raw, total, w.bam_out, w.bam_out_cap);
			if (zlen < 0) { fail(ngm_pipeline_last_error()); return false; }
			t_bgzf_gpu_us += (long long) (ngm_bgzf_last_kernel_ms(w.bz) * 1000.0f);
			bgzf_in_bytes += total; bgzf_out_bytes += (unsigned long long) zlen;
		}
	}
	const int n_out = (int) std::max<long long>(1, std::min<long long>(n_chunks, zlen / (2 << 20) + 1));
	b.chunks.resize((size_t) n_out);
	pool.parallel_for(n_out, [&](int lo, int hi) {
		for (int c = lo; c < hi; ++c) {
			const size_t a = (size_t) ((unsigned long long) zlen * (unsigned) c / (unsigned) n_out), e = (size_t) ((unsigned long long) zlen * (unsigned) (c + 1) / (unsigned) n_out);
			b.chunks[c].assign(w.bam_out + a, e - a);
		}
	}, 1);
	t_bgzf_call_us += us_since(tz);
	return true;
}

void Run::worker_main(Worker &w) {
	std::unique_ptr<Batch> b;
	for (;;) {
		auto tw = Clock::now();
		if (!q_in->pop(b)) break;
		t_wait_us += us_since(tw);
		auto tp = Clock::now();
		PairTurn turn{w.m, o.paired != 0};   // (passed on at the end of this round of the loop unless a map call has run)
		if (failed) { ngm_mapper_set_batch_seq(w.m, b->seq); continue; }
		if (parse_batch(w, *b) && o.paired) check_mate_names(*b);
		ngm_mapper_set_batch_seq(w.m, b->seq);
		if (failed) continue;
		if (route.gpu_sam) gpu_text_route(w, b, turn, tp); else host_format_route(w, b, turn, tp);
	}
}

// ---- the writer: batches in input order, large writes ---------------------------------------------------------------------------
void Run::writer_main() {
	uint64_t next = 0;
	for (;;) {
		std::unique_ptr<Batch> b;
		{
			std::unique_lock<std::mutex> lk(out_mu);
			next_write = next;
			out_cv.notify_all();
			{ std::lock_guard<std::mutex> lk2(text_mu); }   // (a worker between its predicate and its wait holds text_mu: it sees the new value or the notify)
			text_cv.notify_all();
			out_cv.wait(lk, [&] { return out_ready.count(next) || workers_done; });
			auto it = out_ready.find(next);
			if (it == out_ready.end()) return;  // workers are done and the next batch never came (failure) or everything is written
			b = std::move(it->second);
			out_ready.erase(it);
		}
		out_cv.notify_all();
		const auto t_wr = Clock::now();
		if (b->text) {
			// (the batch's text in k slices written at the same time was tried: one file takes 9-14 GB/s whatever the number of writers,
			// profiles/r03_write_calibration.txt)
			if (b->text_len && !put_all(b->text, b->text_len, out_off)) fail("write error on " + o.out);
			out_off += b->text_len;
			t_write_us += us_since(t_wr);
			{ std::lock_guard<std::mutex> lk(text_mu); text_free.push_back(TextBuf{b->text, b->text_cap}); }
			text_cv.notify_one();
		} else {
			// one writer: buffered writes to one file serialise on its inode lock anyway, and pool threads queueing there (64 of
			// them, 500 chunks per batch) burn more system time than the copies take (measured: 32 s of it for 4.2 GB)
			for (const std::string &c : b->chunks) { if (!c.empty() && !put_all(c.data(), c.size(), out_off)) fail("write error on " + o.out); out_off += c.size(); }
			t_write_us += us_since(t_wr);
			std::lock_guard<std::mutex> lk(spare_mu);
			spare_chunks.push_back(std::move(b->chunks));
		}
		n_total += b->n_total; n_mapped += b->n_mapped; n_written += b->n_written; n_read += (size_t) b->n;
		++next;
	}
}

// --sort: every record of the run is in the sorter now.  One sort, then the sorted stream chunk by chunk as BGZF members behind the
// header members, the end-of-file member behind them, and the index next to the file
void Run::finish_sort() {
	const auto t_sort = Clock::now();
	const uint64_t first_member = out_off;
	size_t cap = (size_t) 40 << 20;
	char *buf = (char *) ngm_host_alloc(cap);
	if (!buf) fail(ngm_pipeline_last_error());
	else if (const int rc = ngm_bam_sort_finish(sorter, (int) contig_names.size()); rc < 0) fail(pipeline_error(rc));
	while (!failed) {
		const long long got = ngm_bam_sort_next(sorter, buf, cap);
		if (got < 0) { fail(pipeline_error(got)); break; }
		if (got == 0) break;
		if ((size_t) got > cap) {
			ngm_host_free(buf);
			cap = (size_t) got;
			buf = (char *) ngm_host_alloc(cap);
			if (!buf) { fail(ngm_pipeline_last_error()); break; }
			continue;
		}
		if (!put_all(buf, (size_t) got, out_off)) { fail("write error on " + o.out); break; }
		out_off += (uint64_t) got;
	}
	ngm_host_free(buf);
	if (!failed) {
		const long long ilen = ngm_bam_sort_index(sorter, first_member, nullptr, 0);
		std::string bai(ilen > 0 ? (size_t) ilen : 0, '\0');
		if (ilen < 0 || ngm_bam_sort_index(sorter, first_member, &bai[0], bai.size()) != ilen) fail(pipeline_error(ilen));
		else {
			const std::string bai_path = o.out + ".bai";
			FILE *bf = fopen(bai_path.c_str(), "wb");
			if (!bf || fwrite(bai.data(), 1, bai.size(), bf) != bai.size() || fclose(bf) != 0) fail("write error on " + bai_path);
		}
	}
	if (failed) return;
	uint64_t sc[5] = {0, 0, 0, 0, 0};
	float sm[5] = {0, 0, 0, 0, 0};
	(void) ngm_bam_sort_stats(sorter, sc, sm);
	infof("MAIN", "Sorted on the GPU: %llu records (%.1f MiB held in GPU memory); kernels: keys %.2f ms, sort %.2f ms, gather %.2f ms, deflate %.2f ms, index %.2f ms; "
			"%llu members in %llu chunks, %llu bins; %.3f s after the last batch", (unsigned long long) sc[0], (double) sc[1] / (double) (1 << 20), sm[0], sm[1], sm[2], sm[3], sm[4],
			(unsigned long long) sc[2], (unsigned long long) sc[3], (unsigned long long) sc[4], span_s(t_sort));
	if (o.markdup) {
		uint64_t dc[6] = {0, 0, 0, 0, 0, 0};
		float dm[2] = {0, 0};
		if (ngm_bam_sort_markdup_stats(sorter, dc, dm) < 0) { fail(ngm_pipeline_last_error()); return; }
		infof("SORT", "Duplicates marked on the GPU: %llu records examined, %llu pairs, %llu fragments, %llu duplicate pairs, %llu duplicate fragments, %llu records newly marked; "
				"kernels: marking %.2f ms, sorts %.2f ms", (unsigned long long) dc[0], (unsigned long long) dc[1], (unsigned long long) dc[2], (unsigned long long) dc[3],
				(unsigned long long) dc[4], (unsigned long long) dc[5], dm[0], dm[1]);
	}
}

// --coverage, --snp: every batch has added its records.  The counters become text chunk by chunk on the GPU (finish, then next until it
// returns 0; more than the buffer holds: nothing was copied, ask again with a larger one); the text is streamed into the file
template <class Finish, class Next> void Run::drain(Finish finish, Next next, FILE *&file, const std::string &path, const char *tag, const std::function<void(const char *, size_t)> &tap) {
	FILE *f = file;
	size_t cap = (size_t) 8 << 20;
	std::vector<char> buf(cap);
	if (finish() < 0) fail(tag + std::string(ngm_pipeline_last_error()));
	while (!failed) {
		const long long got = next(buf.data(), cap);
		if (got < 0) { fail(tag + std::string(ngm_pipeline_last_error())); break; }
		if (got == 0) break;
		if ((size_t) got > cap) { cap = (size_t) got; buf.resize(cap); continue; }
		if (fwrite(buf.data(), 1, (size_t) got, f) != (size_t) got) { fail("write error on " + path); break; }
		if (tap) tap(buf.data(), (size_t) got);   // (whole lines)
	}
	file = nullptr;
	if (fclose(f) != 0) fail("write error on " + path);
}

void Run::drain_side_outputs() {
	if (coverage && !failed) {
		const auto t_cov = Clock::now();
		drain([&] { return ngm_coverage_finish(coverage); }, [&](char *p, size_t n) { return ngm_coverage_next(coverage, p, n); }, coverage_file, o.coverage, "--coverage: ");
		if (!failed) {
			uint64_t cc[4] = {0, 0, 0, 0};
			float cms[4] = {0, 0, 0, 0};
			(void) ngm_coverage_stats(coverage, cc, cms);
			infof("MAIN", "Coverage on the GPU: %llu alignments, %llu covered bases, %llu runs, %llu bytes of bedGraph; kernels: add %.2f ms, scan %.2f ms, runs %.2f ms, text %.2f ms; "
					"%.3f s after the last batch", (unsigned long long) cc[0], (unsigned long long) cc[1], (unsigned long long) cc[2], (unsigned long long) cc[3], cms[0], cms[1], cms[2], cms[3], span_s(t_cov));
		}
	}
	if (snp && !failed) {
		const auto t_snp = Clock::now();
		// --count with --snp: every position the VCF calls, whatever the ALT, joins the count's mask -- read off the lines as they are written
		std::vector<int32_t> m_ref, m_pos;
		std::map<std::string, int32_t> by_name;
		if (counter) for (size_t i = 0; i < contig_names.size(); ++i) by_name.emplace(contig_names[i], (int32_t) i);
		std::function<void(const char *, size_t)> tap;
		// (the pieces are cut wherever they are cut: a line is taken when its end has come, so nothing rests on how the text is framed; a data
		// line that does not give a contig of the reference and a position fails the run instead of leaving a hole in the mask)
		std::string pending, bad_line;
		auto take_line = [&](const char *p, const char *end) {
			if (p == end || *p == '#') return;
			const char *t1 = (const char *) memchr(p, '\t', (size_t) (end - p));
			const auto it = t1 ? by_name.find(std::string(p, t1)) : by_name.end();
			long long pos1 = 0;
			for (const char *d = t1 ? t1 + 1 : end; d < end && *d >= '0' && *d <= '9' && pos1 < (1ll << 40); ++d) pos1 = pos1 * 10 + (*d - '0');
			if (it == by_name.end() || pos1 <= 0 || pos1 > 2147483647ll) { if (bad_line.empty()) bad_line.assign(p, end); return; }
			m_ref.push_back(it->second); m_pos.push_back((int32_t) (pos1 - 1));
		};
		if (counter) tap = [&](const char *p, size_t n) {
			for (const char *e = p + n; p < e;) {
				const char *nl = (const char *) memchr(p, '\n', (size_t) (e - p));
				if (!nl) { pending.append(p, e); break; }
				if (pending.empty()) take_line(p, nl);
				else { pending.append(p, nl); take_line(pending.data(), pending.data() + pending.size()); pending.clear(); }
				p = nl + 1;
			}
		};
		drain([&] { return ngm_snp_finish(snp); }, [&](char *p, size_t n) { return ngm_snp_next(snp, p, n); }, snp_file, o.snp, "--snp: ", tap);
		if (counter && !pending.empty()) take_line(pending.data(), pending.data() + pending.size());   // (a last line without its newline)
		if (counter && !failed && !bad_line.empty()) fail("--count: a line of " + o.snp + " gives no position of the reference for the mask: " + bad_line.substr(0, 80));
		if (counter && !failed && ngm_count_mask(counter, m_ref.data(), m_pos.data(), m_ref.size()) < 0) fail(std::string("--count: ") + ngm_pipeline_last_error());
		if (!failed) {
			uint64_t sc[5] = {0, 0, 0, 0, 0};
			float sms[4] = {0, 0, 0, 0};
			(void) ngm_snp_stats(snp, sc, sms);
			infof("MAIN", "SNPs on the GPU: %llu alignments, %llu mismatching bases counted, %llu calls, %llu bytes of VCF; kernels: add %.2f ms, scan %.2f ms, flag %.2f ms, text %.2f ms; "
					"%llu covered bases; %.3f s after the last batch", (unsigned long long) sc[0], (unsigned long long) sc[1], (unsigned long long) sc[2], (unsigned long long) sc[3], sms[0], sms[1], sms[2], sms[3],
					(unsigned long long) sc[4], span_s(t_snp));
		}
	}
	if (counter && !failed) {   // (behind --snp: its calls are the mask)
		const auto t_count = Clock::now();
		std::vector<int64_t> six(count_regions.size() * 6, 0);
		if (ngm_count_finish(counter) < 0 || ngm_count_read(counter, six.data(), count_regions.size()) < 0) fail(std::string("--count: ") + ngm_pipeline_last_error());
		else {
			std::vector<const char *> names;
			for (const std::string &n : contig_names) names.push_back(n.c_str());
			const std::string text = ngm::cnt::serialise(count_regions, names.data(), six.data());
			if (fwrite(text.data(), 1, text.size(), count_file) != text.size()) fail("write error on " + o.count_out);
		}
		FILE *f = count_file;
		count_file = nullptr;
		if (fclose(f) != 0) fail("write error on " + o.count_out);
		if (!failed) {
			uint64_t kc[5] = {0, 0, 0, 0, 0};
			float kms[2] = {0, 0};
			(void) ngm_count_stats(counter, kc, kms);
			infof("MAIN", "Conversions on the GPU: %llu alignments, %llu of them in a region, %llu eligible columns, %llu conversions, %llu masked positions in %zu regions; "
					"kernels: add %.2f ms, reduce %.2f ms; %.3f s after the last batch", (unsigned long long) kc[0], (unsigned long long) kc[1], (unsigned long long) kc[2], (unsigned long long) kc[3],
					(unsigned long long) kc[4], count_regions.size(), kms[0], kms[1], span_s(t_count));
		}
	}
	if (methyl && !failed) {
		const auto t_methyl = Clock::now();
		drain([&] { return ngm_methyl_finish(methyl); }, [&](char *p, size_t n) { return ngm_methyl_next(methyl, p, n); }, methyl_file, o.methyl, "--methyl: ");
		if (!failed) {
			uint64_t mc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			float mms[4] = {0, 0, 0, 0};
			(void) ngm_methyl_stats(methyl, mc, mms);
			auto pct = [](uint64_t m, uint64_t u) { return m + u ? 100.0 * (double) m / (double) (m + u) : 0.0; };
			infof("MAIN", "Methylation on the GPU: %llu alignments, %llu lines; kernels: add %.2f ms, flag %.2f ms, select %.2f ms, text %.2f ms; %.3f s after the last batch",
					(unsigned long long) mc[0], (unsigned long long) mc[1], mms[0], mms[1], mms[2], mms[3], span_s(t_methyl));
			infof("METHYL", "CpG %llu methylated, %llu unmethylated (%.2f%%); CHG %llu, %llu (%.2f%%); CHH %llu, %llu (%.2f%%)", (unsigned long long) mc[2], (unsigned long long) mc[3],
					pct(mc[2], mc[3]), (unsigned long long) mc[4], (unsigned long long) mc[5], pct(mc[4], mc[5]), (unsigned long long) mc[6], (unsigned long long) mc[7], pct(mc[6], mc[7]));
		}
	}
}

// ---- the final report -----------------------------------------------------------------------------------------------------------
void Run::report(double secs) {
	const int pool_size = ngm::ThreadPool::instance().size();
	// src/NGM_main.cpp:150-160: reads that were read but never reached the writer's counters ("discarded": empty reads, and the pairs the
	// reference loses -- ngm_mapper_set_reference_score_buffer) are listed when there are any
	const size_t n_discarded = n_read > n_total ? n_read - n_total : 0;
	if (n_discarded) infof("MAIN", "Done (%zu reads mapped (%.2f%%), %zu reads not mapped (%zu discarded), %zu lines written)", n_mapped,
			100.0 * n_mapped / std::max<size_t>(1, n_total + n_discarded), n_total - n_mapped + n_discarded, n_discarded, n_written);
	else infof("MAIN", "Done (%zu reads mapped (%.2f%%), %zu reads not mapped, %zu lines written)", n_mapped,
			n_total ? 100.0 * n_mapped / n_total : 0.0, n_total - n_mapped, n_written);
	{
		// this process's share of the mapping statistics
		int64_t sv[8] = {(int64_t) n_read, (int64_t) n_mapped, (int64_t) (n_read - n_mapped), (int64_t) n_written, (int64_t) pair_stat[0].load(), (int64_t) pair_stat[1].load(),
				(int64_t) pair_stat[2].load(), (int64_t) (pair_stat[0].load() - pair_stat[1].load())};
		if (o.stats_fd >= 0) {   // a shard process: the parent sums the shards' vectors
			if (write(o.stats_fd, sv, sizeof(sv)) != (ssize_t) sizeof(sv)) info("MAIN", "warning: could not hand the statistics to the parent process");
			close(o.stats_fd);
		}
		if (stats_comm_thread.joinable()) stats_comm_thread.join();
		if (stats_comm) {
			const auto t_ar = Clock::now();
			int64_t all[8];
			memcpy(all, sv, sizeof(all));
			if (ngm_stats_allreduce(stats_comm, all) == 0) {
				if (o.shard_i == 0) {
					infof("MAIN", "Statistics all-reduce over %d GPUs (RCCL, %.0f us): %lld reads, %lld mapped, %lld not mapped, %lld lines written; %lld pairs with both mates mapped, %lld of them broken, mean insert size %.1f",
							o.shard_n, std::chrono::duration<double, std::micro>(Clock::now() - t_ar).count(), (long long) all[0], (long long) all[1], (long long) all[2], (long long) all[3],
							(long long) all[4], (long long) all[5], all[7] > 0 ? (double) all[6] / (double) all[7] : 0.0);
				}
			} else info("MAIN", std::string("warning: statistics all-reduce failed: ") + ngm_pipeline_last_error());
			ngm_stats_comm_destroy(stats_comm);
		} else if (!stats_comm_error.empty() && o.shard_i == 0) info("MAIN", "note: no RCCL communicator for the statistics (" + stats_comm_error + "); the parent process sums them");
	}
	infof("MAIN", "Mapping pass: %.3f s, %.0f reads/s (%zu GPU(s) x %d worker(s), %d host threads, %s input)", secs, n_total / std::max(1e-9, secs),
			o.devices.size(), o.workers, pool_size, plain ? (mf0.owned ? "gzip FASTQ inflated to memory" : "memory-mapped plain FASTQ") : "serial reader");
	infof("MAIN", "GPU kernels: %.3f s of the %.3f s mapping pass (%.0f %%; candidate search, gathers, score, select, align, traceback by HIP events)",
			t_gpu_us / 1e6, secs, 100.0 * (t_gpu_us / 1e6) / std::max(1e-9, secs));
	if (!route.gpu_sam) {
		infof("MAIN", "Records%s formatted on the host pool: %.3f s of thread time = %.0f %% of %d threads x %.3f s", (o.bam && !route.gpu_bgzf) ? " + BGZF blocks" : "", t_format_cpu_us / 1e6,
				100.0 * (t_format_cpu_us / 1e6) / std::max(1e-9, pool_size * secs), pool_size, secs);
	}
	if (route.gpu_bgzf) {
		infof("MAIN", "BGZF blocks written by the GPU: %.1f MB of records -> %.1f MB, %.3f s of kernels, %.3f s inside the calls (copies to and from page-locked memory, both transfers, the kernels)",
				bgzf_in_bytes.load() / 1e6, bgzf_out_bytes.load() / 1e6, t_bgzf_gpu_us / 1e6, t_bgzf_call_us / 1e6);
	}
	if (route.gpu_sam) { infof("MAIN", "%s on the GPU: %.3f s of kernels (included above)", o.bam ? "BAM records and their BGZF blocks written" : "SAM text assembled", t_sam_gpu_us / 1e6); }
	infof("MAIN", "Input to output: %.3f s (estimation pass + mapping pass, first input byte to output closed)", span_s(t_input));
	if (getenv("NGM_HIP_HOST_TIMING")) {
		infof("MAIN", "Before the mapping pass, s: input mapped + record index + read lengths %.3f | sensitivity estimate %.3f | header, mappers, page-locked buffers %.3f",
				span_s(t_input, t_indexed), span_s(t_indexed, t_estimated), span_s(t_estimated, t_start));
		infof("MAIN", "Worker time summed over %zu workers, s: waiting for input %.3f | parse + pack %.3f | map (GPU + library host stages) %.3f | format %.3f",
				workers.size(), t_wait_us / 1e6, t_parse_us / 1e6, t_map_us / 1e6, t_format_us / 1e6);
		struct timespec cpu1;
		clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &cpu1);
		struct rusage ru1;
		getrusage(RUSAGE_SELF, &ru1);
		auto tv = [](const timeval &a, const timeval &b) { return (double) (b.tv_sec - a.tv_sec) + 1e-6 * (double) (b.tv_usec - a.tv_usec); };
		infof("MAIN", "Mapping pass, process totals: CPU %.2f s (user %.2f, system %.2f), page faults %ld minor / %ld major, context switches %ld voluntary / %ld involuntary",
				(double) (cpu1.tv_sec - cpu0.tv_sec) + 1e-9 * (double) (cpu1.tv_nsec - cpu0.tv_nsec), tv(ru0.ru_utime, ru1.ru_utime), tv(ru0.ru_stime, ru1.ru_stime),
				ru1.ru_minflt - ru0.ru_minflt, ru1.ru_majflt - ru0.ru_majflt, ru1.ru_nvcsw - ru0.ru_nvcsw, ru1.ru_nivcsw - ru0.ru_nivcsw);
		infof("MAIN", "Pool thread time inside the stages, s: parse + pack %.3f | format %.3f | output copies %.3f (writer wall %.3f)",
				t_parse_cpu_us / 1e6, t_format_cpu_us / 1e6, t_write_cpu_us / 1e6, t_write_us / 1e6);
	}
	report_search_paths();
}

// the counters of the mappers, summed over the workers
void Run::report_search_paths() {
	if (o.argos) {
		uint64_t ac[4] = {0, 0, 0, 0}, ap[2] = {0, 0};
		for (Worker &w : workers) {
			uint64_t c4[4], c2[2];
			if (ngm_mapper_argos_counters(w.m, c4) == 0) for (int x = 0; x < 4; ++x) ac[x] += c4[x];
			if (ngm_mapper_argos_path_counters(w.m, c2) == 0) for (int x = 0; x < 2; ++x) ap[x] += c2[x];
		}
		const double nl = (double) std::max<uint64_t>(1, ac[0] + ac[1] + ac[2]);
		infof("MAIN", "Argos order classes: U %llu (%.3f %%), S %llu (%.3f %%), H %llu (%.3f %%); %llu entries written; long-list path %llu reads; order by position (candidate order unknown) %llu reads",
				(unsigned long long) ac[0], 100.0 * ac[0] / nl, (unsigned long long) ac[1], 100.0 * ac[1] / nl, (unsigned long long) ac[2], 100.0 * ac[2] / nl,
				(unsigned long long) ac[3], (unsigned long long) ap[0], (unsigned long long) ap[1]);
	}
	uint64_t pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (Worker &w : workers) { uint64_t c8[8]; if (ngm_mapper_path_counters(w.m, c8) == 0) for (int x = 0; x < 8; ++x) pc[x] += c8[x]; }
	const double nr = (double) std::max<uint64_t>(1, pc[0]);
	infof("MAIN", "Candidate search: %llu reads, %.2f candidates per read; heavy-read kernel for %llu reads (%.3f %%), exact search with the table in LDS for %llu (%.3f %%), in global memory for %llu (%.3f %%)",
			(unsigned long long) pc[0], pc[1] / nr, (unsigned long long) pc[7], 100.0 * pc[7] / nr, (unsigned long long) pc[2], 100.0 * pc[2] / nr, (unsigned long long) pc[3], 100.0 * pc[3] / nr);
	uint64_t hc[4] = {0, 0, 0, 0};
	for (Worker &w : workers) { uint64_t c4[4]; if (ngm_mapper_heavy_counters(w.m, c4) == 0) for (int x = 0; x < 4; ++x) hc[x] += c4[x]; }
	infof("MAIN", "Heavy-read kernel: %llu second passes, %llu table passes started over, %llu reads sent on to the exact kernels; table pool regrown %llu times",
			(unsigned long long) hc[0], (unsigned long long) hc[1], (unsigned long long) hc[2], (unsigned long long) hc[3]);
	uint64_t by_table = 0;
	for (Worker &w : workers) { uint64_t c2 = 0; if (ngm_mapper_order_table_reads(w.m, &c2) == 0) by_table += c2; }
	infof("MAIN", "Candidate order replay: %llu reads, %llu of them beyond the LDS replay (exact replay through buckets in global memory, %llu of them with a table there); order left undetermined for %llu reads",
			(unsigned long long) pc[4], (unsigned long long) pc[5], (unsigned long long) by_table, (unsigned long long) pc[6]);
	if (o.paired && o.ref_score_buffer > 0) {
		uint64_t lost = 0;
		for (Worker &w : workers) { uint64_t c2 = 0; if (ngm_mapper_lost_pairs(w.m, &c2) == 0) lost += c2; }
		infof("MAIN", "Pairs lost as NextGenMap loses them (first mate's last score fills the %d-entry score buffer, second mate without candidates; src/ScoreBuffer.cpp:196, :519-523): %llu",
				o.ref_score_buffer, (unsigned long long) lost);
	}
}

void Run::teardown() {
	for (Worker &w : workers) { ngm_mapper_destroy(w.m); ngm_host_free(w.rows); ngm_host_free(w.qrows); ngm_host_free(w.names); ngm_host_free(w.meta); ngm_host_free(w.polya);
		ngm_bgzf_destroy(w.bz); ngm_host_free(w.bam_raw); ngm_host_free(w.bam_out); }
	ngm_bam_sort_destroy(sorter);
	ngm_coverage_destroy(coverage); ngm_snp_destroy(snp); ngm_count_destroy(counter); ngm_methyl_destroy(methyl);
	for (FILE *f : {coverage_file, snp_file, count_file, methyl_file}) if (f) fclose(f);
	for (TextBuf &t : text_free) ngm_host_free(t.p);
	ngm_pair_state_destroy(pair_state);
	for (ngm_ref *r2 : refs) ngm_ref_destroy(r2);
}

}  // namespace

int main(int argc, char **argv) {
	// every batch allocates and frees a few hundred MB in MB-sized pieces from ~64 threads (output chunks, record views): with
	// glibc's defaults each of them is an mmap / page-fault / munmap cycle, and the kernel's address-space lock serialises the
	// formatter threads (measured: 55 ms per 256 k reads instead of ~2).  Keep that memory in the heap.
	mallopt(M_MMAP_THRESHOLD, 32 << 20);
	mallopt(M_TRIM_THRESHOLD, 1 << 30);
	mallopt(M_TOP_PAD, 64 << 20);
	Run R;
	R.t_process = std::chrono::steady_clock::now();
	R.o = parse(argc, argv);
	const Opts &o = R.o;
	R.refuse_by_input_format();
	R.read_count_regions();
	if (o.shard_output && (o.devices.size() > 1 || getenv("NGM_HIP_SHARD_SINGLE")) && o.shard_n == 1 && o.stats_fd < 0 && !o.out.empty() && !(o.qry.empty() && o.qry1.empty())) return run_sharded(argc, argv, o);   // (a shard process has its parent's --stats-fd)
	R.join_communicator();
	// bisulfite mapping: the index holds every reference k-mer, the run's kmer_skip applies to the reads (src/PrefixTable.cpp:199-207, src/CS.cpp:556-560)
	R.rp = ngm_ref_params{o.kmer, o.bs_mapping ? 0 : o.kmer_skip, o.bin_size};
	info("MAIN", "NextGenMap-compatible HIP backend (gfx950)");
	if (o.bs_mapping) info("MAIN", "BS mapping enabled. Max. number of A/T per k-mer set to " + std::to_string(o.bs_cutoff));
	// one GPU: keep every host thread (this one, the workers, the pool) on the socket the GPU hangs on -- the parse / select /
	// format stages run twice as fast there as spread over both sockets of the host
	if (o.devices.size() == 1) {
		const int cpus = ngm_host_pin_to_device_node(o.device);
		if (cpus > 0) info("MAIN", "Host threads pinned to the " + std::to_string(cpus) + " CPUs of the GPU's NUMA node");
	}
	R.route = output_route(o);
	R.request_pinned_early();
	R.load_reference();
	R.first_input = o.qry1.empty() ? o.qry : o.qry1;  // parser1: what the estimation pass reads (ReadProvider.cpp:201)
	if (R.first_input.empty()) { ngm_ref_destroy(R.ref); return 0; }  // index only, like `ngm -r ref.fa`
	if (o.out.empty()) die("no output file given (-o/--output)");
	R.scan_input();
	R.estimate_sensitivity();
	R.write_header();
	R.create_mappers_and_side_outputs();
	R.setup_formatter();

	// ---- the pipeline: splitter -> workers -> writer ----------------------------------------------------------------------------
	R.q_in.reset(new BoundedQueue<std::unique_ptr<Batch>>(R.workers.size() + 2));
	std::thread splitter([&R] { R.splitter_main(); });
	R.take_pinned();
	R.t_start = std::chrono::steady_clock::now();   // the mapping pass: mappers and page-locked buffers exist, the splitter has begun to cut batches
	std::thread writer([&R] { R.writer_main(); });
	if (getenv("NGM_HIP_PROFILE")) prof::start();  // the mapping pass only
	clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &R.cpu0);
	getrusage(RUSAGE_SELF, &R.ru0);
	{
		std::vector<std::thread> th;
		for (Worker &w : R.workers) th.emplace_back([&R, pw = &w] { R.worker_main(*pw); });
		for (auto &t : th) t.join();
	}
	splitter.join();
	if (R.estimate_thread.joinable()) R.estimate_thread.join();   // (it finished long ago unless the input is a handful of reads; the reference it uses is released below)
	{ std::lock_guard<std::mutex> lk(R.out_mu); R.workers_done = true; }
	R.out_cv.notify_all();
	writer.join();
	if (R.sorter && !R.failed) R.finish_sort();
	R.drain_side_outputs();
	if (o.bam && o.shard_i == o.shard_n - 1) { std::string z; ngm::bam::bgzf_eof(z); if (!R.put_all(z.data(), z.size(), R.out_off)) R.fail("write error on " + o.out); R.out_off += z.size(); }   // (--shard: the end-of-file block travels with the last shard)
	if (close(R.out_fd) != 0) R.fail("write error on " + o.out);
	if (R.failed) die(R.fail_msg);
	R.report(span_s(R.t_start));
	if (const char *pf = getenv("NGM_HIP_PROFILE")) prof::dump(pf);
	R.teardown();
	return 0;
}
