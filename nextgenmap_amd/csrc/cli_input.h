// cli_input.h -- the input side of `ngm-hip`: the serial FASTA / FASTQ reader, a whole input file in memory (plain, .gz and BGZF
// inflated, SAM / BAM), the record indexes the splitter cuts batches from, a batch on its way through the pipeline, and the queue
// between the splitter and the workers.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>

#include "bam_input.h"
#include "bgzf_inflate_device.h"
#include "cli_format.h"
#include "cli_options.h"
#include "gz_inflate.h"
#include "thread_pool.h"

namespace ngm::cli {

struct Read { std::string name, seq, qual; uint8_t unit = 0; };   // unit: --broken-pairs (1 a read without its mate, 2 the placeholder in the mate's row, 4 the pair's 0x40 / 0x80 flags are swapped)

// FASTA / FASTQ reader with kseq semantics: name = header up to the first white space, multi-line records
class SeqReader {
public:
	explicit SeqReader(const char *path) : f_(gzopen(path, "rb")) { if (f_) gzbuffer(f_, 1 << 20); }
	~SeqReader() { if (f_) gzclose(f_); }
	bool ok() const { return f_ != nullptr; }
	bool next(Read &r) {
		std::string line;
		if (!have_header_) { while (getline(line)) if (!line.empty() && (line[0] == '@' || line[0] == '>')) { header_ = line; have_header_ = true; break; } }
		if (!have_header_) return false;
		const bool fastq = header_[0] == '@';
		size_t e = 1;
		while (e < header_.size() && header_[e] != ' ' && header_[e] != '\t') ++e;
		r.name.assign(header_, 1, e - 1);
		r.seq.clear();
		r.qual.clear();
		have_header_ = false;
		while (getline(line)) {
			if (fastq && !line.empty() && line[0] == '+') break;
			if (!fastq && !line.empty() && (line[0] == '>' || line[0] == '@')) { header_ = line; have_header_ = true; break; }
			r.seq += line;
		}
		if (fastq) {
			while (r.qual.size() < r.seq.size() && getline(line)) r.qual += line;
			if (r.qual.size() != r.seq.size()) { fprintf(stderr, "[ngm-hip] error: Error while parsing read: sequence and quality lengths differ (%s)\n", r.name.c_str()); exit(1); }
		}
		return true;
	}

private:
	bool getline(std::string &out) {
		out.clear();
		char buf[65536];
		bool any = false;
		while (gzgets(f_, buf, sizeof(buf))) {
			any = true;
			size_t n = strlen(buf);
			const bool eol = n && buf[n - 1] == '\n';
			while (n && (buf[n - 1] == '\n' || buf[n - 1] == '\r')) --n;
			out.append(buf, n);
			if (eol) break;
		}
		return any;
	}
	gzFile f_;
	std::string header_;
	bool have_header_ = false;
};

// ---- input: records (Rec, cli_format.h) as views into the mapped file (plain FASTQ) or into storage owned by the batch (serial reader) ----
inline void pack_row(const Read &r, int q, char *row) { (void) ngm::trim::pack_row(r.seq.data(), r.seq.size(), q, row); }  // IParser.h:59-121

// a whole file mapped read-only; plain() = not gzip and made of 4-line FASTQ records (checked on the first records)
struct MappedFile {
	const char *p = nullptr;
	size_t n = 0, map_len = 0;   // n: the bytes that hold records (white space at the end of the file is not a record: kseq skips it too)
	int fd = -1;
	char *owned = nullptr;        // gzip input: the inflated text lives here instead of in a file mapping
	size_t owned_map = 0;         // != 0: `owned` is an anonymous mapping of this many bytes (gz_inflate.h), else malloc'ed
	int device = 0;               // BGZF input: the GPU that inflates it
	int format = ngm::bamin::kFastx;   // of the (inflated) bytes: ngm::bamin::Format
	bool open(const char *path) {
		fd = ::open(path, O_RDONLY);
		if (fd < 0) return false;
		struct stat st;
		if (fstat(fd, &st) != 0 || st.st_size == 0) return false;
		unsigned char magic[2] = {0, 0};
		if (st.st_size >= 2 && pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b) return inflate_all(path);
		n = map_len = (size_t) st.st_size;
		void *m = mmap(nullptr, map_len, PROT_READ, MAP_PRIVATE, fd, 0);
		if (m == MAP_FAILED) { p = nullptr; return false; }
		p = (const char *) m;
		madvise(m, map_len, MADV_SEQUENTIAL);
		trim();
		return n > 0;
	}
	// (a BAM file is binary: its last bytes belong to its last record)
	void trim() { format = ngm::bamin::detect(p, n, true); if (format == ngm::bamin::kBam) return; while (n > 0 && (p[n - 1] == '\n' || p[n - 1] == '\r' || p[n - 1] == ' ' || p[n - 1] == '\t')) --n; }
	// .gz input: inflated ONCE into memory (zlib, one thread per file -- the two files of a pair at the same time) and then read
	// like a mapped plain file by all pool threads, instead of twice through a line-by-line reader (estimation pass, mapping pass).
	// Inputs that inflate to more than 64 GB per file go through the serial reader.
	// BGZF (every BAM, every file written by bgzip): the members are independent, the GPU inflates them (bgzf_inflate_device.h) into the
	// one reserved range a .gz input lives in.  false: not BGZF, or a member the GPU refuses -- the file then takes the host's route
	// below, whose message the user sees.  NGM_HIP_BGZF_INFLATE_HOST=1 forces that route.
	bool inflate_bgzf(const char *path, size_t cap_max) {
		if (getenv("NGM_HIP_BGZF_INFLATE_HOST")) return false;
		struct stat st;
		if (fstat(fd, &st) != 0 || st.st_size < 28) return false;
		unsigned char head[4];
		if (pread(fd, head, 4, 0) != 4 || head[2] != 8 || head[3] != 4) return false;   // (BGZF: deflate, FLG = FEXTRA alone)
		const size_t zn = (size_t) st.st_size;
		void *zm = mmap(nullptr, zn, PROT_READ, MAP_PRIVATE, fd, 0);
		if (zm == MAP_FAILED) return false;
		// the first member carries the BC subfield, wherever among its subfields: the walk over the chain below looks for it the same way
		if (!ngm::inflate::first_member_is_bgzf((const uint8_t *) zm, zn)) { munmap(zm, zn); return false; }
		madvise(zm, zn, MADV_SEQUENTIAL);
		const size_t total = ngm_bgzf_inflated_size(zm, zn);
		if (total == (size_t) -1 || total == 0 || total > cap_max) { munmap(zm, zn); return false; }
		const size_t res = ((total + 320 + 4095) & ~(size_t) 4095) + ((size_t) 2 << 20);
		void *om = mmap(nullptr, res, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
		if (om == MAP_FAILED) { munmap(zm, zn); return false; }
		// (the first touch of the text's pages is the kernel's, on a thread of its own, as for a .gz input: gz_inflate.h)
		std::thread toucher([om, total] {
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
			for (size_t o = 0; o < total; o += (size_t) 4 << 20) if (madvise((char *) om + o, std::min<size_t>((size_t) 4 << 20, ((total - o) + 4095) & ~(size_t) 4095), MADV_POPULATE_WRITE) != 0) return;
		});
		ngm_bgzf *z = ngm_bgzf_create(device);
		const long long got = z ? ngm_bgzf_inflate(z, zm, zn, om, total) : -1;
		const float ms = z ? ngm_bgzf_last_kernel_ms(z) : 0.f;
		if (z) ngm_bgzf_destroy(z);
		toucher.join();
		munmap(zm, zn);
		if (got != (long long) total) {
			info("INPUT", std::string("GPU BGZF inflate of ") + path + " failed (" + ngm_pipeline_last_error() + "): reading it on the host");
			munmap(om, res);
			return false;
		}
		static std::atomic<bool> said{false};
		if (!said.exchange(true)) {
			char m[200];
			snprintf(m, sizeof(m), "BGZF blocks inflated on the GPU (%.1f MB of text, kernels %.1f ms)", total / 1e6, ms);
			info("INPUT", m);
		}
		owned = (char *) om; owned_map = res; p = owned; n = total; map_len = 0;
		trim();
		return true;
	}
	bool inflate_all(const char *path) {
		const size_t cap_max = (size_t) 64 << 30;
		if (inflate_bgzf(path, cap_max)) return n > 0;
		{   // (what gz_inflate.h refuses -- a damaged stream, a wrong CRC or length -- falls back to zlib's inflate below)
			char *text = nullptr;
			size_t len = 0, reserved = 0;
			if (ngm::gz::inflate_file(path, &text, &len, &reserved, cap_max)) {
				owned = text; owned_map = reserved; p = text; n = len; map_len = 0;
				trim();
				return n > 0;
			}
		}
		gzFile g = gzopen(path, "rb");
		if (!g) return false;
		gzbuffer(g, 1 << 20);
		size_t cap = (size_t) 256 << 20, len = 0;
		char *buf = (char *) malloc(cap);
		bool ok = buf != nullptr;
		while (ok) {
			if (cap - len < ((size_t) 16 << 20)) {
				if (cap >= cap_max) { ok = false; break; }
				cap = std::min(cap_max, cap * 2);
				char *nb = (char *) realloc(buf, cap);
				if (!nb) { ok = false; break; }
				buf = nb;
			}
			const int got = gzread(g, buf + len, (unsigned) std::min<size_t>(cap - len, (size_t) 1 << 30));
			if (got < 0) { ok = false; break; }
			if (got == 0) break;
			len += (size_t) got;
		}
		gzclose(g);
		if (!ok || len == 0) { free(buf); return false; }
		owned = buf; p = buf; n = len; map_len = 0;
		trim();
		return n > 0;
	}
	void drop_owned() { if (owned_map) munmap(owned, owned_map); else free(owned); owned = nullptr; owned_map = 0; }
	void release() { if (owned) { drop_owned(); p = nullptr; n = 0; } }
	~MappedFile() { if (owned) drop_owned(); else if (p) munmap((void *) p, map_len); if (fd >= 0) close(fd); }
	// touch every page from the pool threads: the page-table entries of a multi-GB input are then set up in parallel instead
	// of one minor fault at a time under the (single) splitter thread
	void prefault() const {
		if (!p) return;
		const size_t step = (size_t) 8 << 20;
		const int chunks = (int) ((n + step - 1) / step);
		std::atomic<unsigned> sink{0};
		ngm::ThreadPool::instance().parallel_for(chunks, [&](int lo, int hi) {
			unsigned acc = 0;
			for (int c = lo; c < hi; ++c) for (size_t o = (size_t) c * step, e = std::min(n, o + step); o < e; o += 4096) acc += (unsigned char) p[o];
			sink += acc;
		}, 1);
	}
	// one 4-line record starting at `at`: sets the views, returns the offset of the next record, or 0 if malformed
	size_t record(size_t at, Rec &r) const {
		const char *b = p + at, *end = p + n;
		if (at >= n || *b != '@') return 0;
		const char *e0 = (const char *) memchr(b, '\n', end - b);
		if (!e0) return 0;
		const char *s = e0 + 1;
		const char *e1 = s < end ? (const char *) memchr(s, '\n', end - s) : nullptr;
		if (!e1) return 0;
		const char *pl = e1 + 1;
		if (pl >= end || *pl != '+') return 0;
		const char *e2 = (const char *) memchr(pl, '\n', end - pl);
		if (!e2) return 0;
		const char *ql = e2 + 1;
		const char *e3 = ql <= end ? (const char *) memchr(ql, '\n', end - ql) : nullptr;
		const char *qe = e3 ? e3 : end;  // the last line may lack its line end
		auto trim = [](const char *a, const char *z) { while (z > a && z[-1] == '\r') --z; return (uint32_t) (z - a); };
		const char *nm = b + 1;
		uint32_t nl = 0;
		const uint32_t hl = trim(nm, e0);
		while (nl < hl && nm[nl] != ' ' && nm[nl] != '\t') ++nl;  // kseq: name = header up to the first white space
		r.name = nm; r.name_len = nl; r.seq = s; r.seq_len = trim(s, e1); r.qual = ql; r.qual_len = trim(ql, qe);
		return (size_t) ((e3 ? e3 + 1 : end) - p);
	}
	bool plain_fastq() const {
		if (n < 2 || ((unsigned char) p[0] == 0x1f && (unsigned char) p[1] == 0x8b)) return false;
		size_t at = 0;
		Rec r;
		for (int i = 0; i < 1000 && at < n; ++i) {
			const size_t nx = record(at, r);
			if (!nx || r.qual_len != r.seq_len) return false;
			at = nx;
		}
		return true;
	}
};

// ---- a batch on its way through the pipeline -------------------------------------------------------------------------
struct Batch {
	uint64_t seq = 0;
	int n = 0;
	// plain input: byte offsets of every kSub-th record in file 0 / file 1 (two-file paired input: records alternate)
	std::vector<size_t> sub0, sub1;
	int n0 = 0, n1 = 0;                 // records from file 0 / file 1
	std::vector<Read> owned;            // serial reader: the records themselves
	std::vector<std::unique_ptr<char[]>> store;   // SAM / BAM input: per sub-range, what the records' views point into where the file does not hold it (decoded bases, qualities + 33, reversed reads)
	std::vector<Rec> recs;
	std::vector<std::string> chunks;    // formatted output, in order
	char *text = nullptr;               // ... or, formatted on the GPU: one piece in a page-locked buffer of the pool
	size_t text_len = 0, text_cap = 0;
	size_t n_total = 0, n_mapped = 0, n_written = 0;
};
constexpr int kSub = 1024;

// ---- record index of a plain FASTQ file, built by all pool threads ----------------------------------------------------
// The file is cut into byte ranges; every range finds its first record (a line that starts with '@' whose second-next line
// starts with '+': in 4-line FASTQ only header lines have that -- a quality line that starts with '@' is followed by a header and a
// sequence), counts its records, and after a prefix sum over the ranges walks them again to note the byte offset of every
// `step`-th record of the FILE and, for the first input file, what ReadProvider's estimation pass collects (read lengths of the
// first 10 000 001 non-empty reads, every 1 000-th of the first 10 000 000 for the sensitivity sample; src/ReadProvider.cpp:201-305).
struct FastqIndex {
	bool ok = false;
	size_t bad_at = 0;                 // !ok: offset of the record that is not a 4-line FASTQ record
	std::string length_error;          // the first read whose sequence and quality lengths differ (IParser.h copyToRead), if any
	int step = kSub;
	std::vector<size_t> sub;           // offset of record 0, step, 2 step, ...; one more entry: the end of the last record
	size_t n_records = 0, n_nonempty = 0;
	size_t max_len = 0, min_len = 9999999, sum_len = 0, count = 0;   // the estimation pass's numbers
	std::vector<Read> sample;
};

inline void build_fastq_index(const MappedFile &f, int step, bool stats, int trim5, FastqIndex &ix) {
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	const int T = (int) std::max<size_t>(1, std::min<size_t>((size_t) pool.size() * 4, f.n >> 20));
	struct Range { size_t start = 0, n_rec = 0, n_ne = 0, bad_at = 0, rec_base = 0, ne_base = 0, max_len = 0, min_len = 9999999, sum_len = 0; bool bad = false; std::string len_err; std::vector<Read> sample; };
	std::vector<Range> rg((size_t) T + 1);
	rg[T].start = f.n;
	auto line_start_after = [&](size_t o) -> size_t {  // first line start at or after o
		if (o == 0 || f.p[o - 1] == '\n') return o;
		const char *c = (const char *) memchr(f.p + o, '\n', f.n - o);
		return c ? (size_t) (c + 1 - f.p) : f.n;
	};
	auto next_line = [&](size_t o) -> size_t { const char *c = o < f.n ? (const char *) memchr(f.p + o, '\n', f.n - o) : nullptr; return c ? (size_t) (c + 1 - f.p) : f.n; };
	pool.parallel_for(T, [&](int lo, int hi) {
		for (int r = lo; r < hi; ++r) {
			size_t at = r == 0 ? 0 : line_start_after(f.n / T * r);
			if (r > 0) {
				// a header line: '@' here and '+' two lines on
				for (; at < f.n; at = next_line(at)) {
					if (f.p[at] != '@') continue;
					const size_t l2 = next_line(next_line(at));
					if (l2 < f.n && f.p[l2] == '+') break;
				}
			}
			rg[r].start = at;
		}
	}, 1);
	for (int r = 1; r <= T; ++r) if (rg[r].start < rg[r - 1].start) rg[r].start = rg[r - 1].start;  // (ranges shorter than a record)
	auto walk = [&](int r, bool second) {
		Range &R = rg[r];
		Rec rec;
		size_t at = R.start, g = R.rec_base, c = R.ne_base;
		const size_t end = rg[r + 1].start;
		while (at < end) {
			const size_t nx = f.record(at, rec);
			if (!nx) { R.bad = true; R.bad_at = at; return; }
			if (!second) {
				if (rec.qual_len != rec.seq_len && R.len_err.empty()) R.len_err.assign(rec.name, rec.name_len);
				++R.n_rec;
				if (rec.seq_len) ++R.n_ne;
			} else {
				if (g % (size_t) step == 0) ix.sub[g / (size_t) step] = at;
				++g;
				if (stats && rec.seq_len) {   // reads without a sequence are not counted (ReadProvider.cpp:236)
					++c;
					if (c <= 10000001) {
						const size_t len = ngm::trim::estimate_len(rec.seq_len, trim5);   // (the parser's read: behind the -5 prefix, before --max-polya)
						R.max_len = std::max(R.max_len, len); R.min_len = std::min(R.min_len, len); R.sum_len += len;
						if (c % 1000 == 0 && c < 10000000) {
							const char *sq = rec.seq, *ql = rec.qual;
							uint32_t sl = rec.seq_len, qn = 0;
							ngm::trim::trim5(trim5, sq, sl, ql, qn);
							R.sample.push_back(Read{std::string(rec.name, rec.name_len), std::string(sq, sl), std::string()});
						}
					}
				}
			}
			at = nx;
		}
		if (at != end) { R.bad = true; R.bad_at = at; }
	};
	pool.parallel_for(T, [&](int lo, int hi) { for (int r = lo; r < hi; ++r) walk(r, false); }, 1);
	for (int r = 0; r < T; ++r) {
		if (rg[r].bad) { ix.ok = false; ix.bad_at = rg[r].bad_at; return; }
		if (!rg[r].len_err.empty() && ix.length_error.empty()) ix.length_error = rg[r].len_err;
		rg[r].rec_base = ix.n_records; rg[r].ne_base = ix.n_nonempty;
		ix.n_records += rg[r].n_rec; ix.n_nonempty += rg[r].n_ne;
	}
	ix.step = step;
	ix.sub.assign((ix.n_records + (size_t) step - 1) / (size_t) step + 1, f.n);
	pool.parallel_for(T, [&](int lo, int hi) { for (int r = lo; r < hi; ++r) walk(r, true); }, 1);
	for (int r = 0; r < T; ++r) {
		ix.max_len = std::max(ix.max_len, rg[r].max_len); ix.min_len = std::min(ix.min_len, rg[r].min_len); ix.sum_len += rg[r].sum_len;
		for (Read &x : rg[r].sample) ix.sample.push_back(std::move(x));
	}
	ix.count = std::min<size_t>(ix.n_nonempty, 10000001);
	ix.ok = true;
}

// ---- the same index for a SAM or BAM input (bam_input.h): one walk over the records.  A BAM's records are found through the chain of
// their block_size fields, which only a serial walk can follow; it reads 36 bytes per record.  !ix.ok: ix.length_error holds the message.
inline void build_record_index(const MappedFile &f, int step, int trim5, FastqIndex &ix) {
	namespace bi = ngm::bamin;
	ix.step = step;
	size_t c = 0;
	auto account = [&](size_t at, const bi::View *v, uint32_t seq_len, auto &&decode) {
		if (ix.n_records % (size_t) step == 0) ix.sub.push_back(at);
		++ix.n_records;
		if (!seq_len) return;   // reads without a sequence are not counted (ReadProvider.cpp:236)
		++ix.n_nonempty;
		if (++c > 10000001) return;
		const size_t len = ngm::trim::estimate_len(seq_len, trim5);
		ix.max_len = std::max(ix.max_len, len); ix.min_len = std::min(ix.min_len, len); ix.sum_len += len;
		if (c % 1000 == 0 && c < 10000000) {
			bi::View w;
			std::vector<char> store;
			if (v) w = *v; else decode(w, store);
			const char *sq = w.seq, *ql = w.qual;
			uint32_t sl = w.seq_len, qn = 0;
			ngm::trim::trim5(trim5, sq, sl, ql, qn);
			ix.sample.push_back(Read{std::string(w.name, w.name_len), std::string(sq, sl), std::string()});
		}
	};
	if (f.format == bi::kBam) {
		const uint8_t *p = (const uint8_t *) f.p;
		if (!bi::bam_walk(p, f.n, [&](size_t at, size_t, uint32_t ls) {
				account(at, nullptr, ls, [&](bi::View &w, std::vector<char> &store) { store.resize(bi::bam_store_bytes(ls) + 1); bi::bam_decode(p, at, w, store.data()); });
			}, &ix.length_error)) return;
	} else {
		std::vector<char> store;
		for (size_t at = 0, next = 0; at < f.n; at = next) {
			if (!bi::sam_is_record(f.p, f.n, at, &next)) continue;
			store.resize(bi::sam_store_bytes(at, next) + 1);
			bi::View v;
			if (!bi::sam_decode(f.p, at, next, v, store.data())) { ix.length_error = "Error while parsing read: sequence and quality lengths differ (" + std::string(v.name, v.name_len) + ")"; return; }
			account(at, &v, v.seq_len, [](bi::View &, std::vector<char> &) {});
		}
	}
	ix.sub.push_back(f.n);
	ix.count = std::min<size_t>(ix.n_nonempty, 10000001);
	ix.ok = true;
}

template <typename T>
class BoundedQueue {
public:
	explicit BoundedQueue(size_t cap) : cap_(cap) {}
	void push(T v) {
		std::unique_lock<std::mutex> lk(mu_);
		cv_push_.wait(lk, [&] { return q_.size() < cap_; });
		q_.push_back(std::move(v));
		cv_pop_.notify_one();
	}
	bool pop(T &v) {  // false: closed and drained
		std::unique_lock<std::mutex> lk(mu_);
		cv_pop_.wait(lk, [&] { return !q_.empty() || closed_; });
		if (q_.empty()) return false;
		v = std::move(q_.front());
		q_.pop_front();
		cv_push_.notify_one();
		return true;
	}
	void close() { { std::lock_guard<std::mutex> lk(mu_); closed_ = true; } cv_pop_.notify_all(); }
private:
	std::mutex mu_;
	std::condition_variable cv_push_, cv_pop_;
	std::deque<T> q_;
	size_t cap_;
	bool closed_ = false;
};

}  // namespace ngm::cli
