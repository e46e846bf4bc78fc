// side_output.h -- the HIP part the run-long side outputs (csrc/coverage.cpp, csrc/snp.cpp, csrc/count.cpp, csrc/methyl.cpp) share: an object's lifetime
// and statistics (Base), the staging of a batch that comes as arrays (Staged), the contigs' names on the device (Names), and the chunked
// finish of a per-base text output -- scan, flags, select, lengths, offsets, text, whole lines (LineStream).  A side output supplies its
// kernels, their argument struct and what it carries from chunk to chunk; DESIGN.md, "A new side output".  Host-only parts: side_host.h.
// LineStream is only there behind NGM_SIDE_LINE_STREAM: rocPRIM makes count.cpp's code object 12 times as large, its first launch 2 ms slower.
#pragma once

#include <cstring>
#include <mutex>
#include <vector>

#include <hip/hip_runtime.h>
#ifdef NGM_SIDE_LINE_STREAM
#include <rocprim/rocprim.hpp>   // (after <cstring>: its texture iterator calls the host's memset)
#endif

#include "device_util.h"
#include "side_host.h"

namespace ngm {
namespace side {

struct Base {
	int device = 0, n_ref = 0;
	mutable std::mutex mu;          // (the statistics take it on a const object)
	hipStream_t st = nullptr;       // non-blocking: the object's own work waits for no mapper
	std::vector<hipEvent_t> ev;
	bool finished = false;
	float ms[4] = {0, 0, 0, 0};     // [0] the add kernels, the mappers' too; the rest is the derived object's
	Buf<unsigned long long> d_tot;  // the totals the kernels count; [0] alignments

	// the stream, the events and the zeroed totals, on the calling thread's device
	bool open(int device_, size_t n_events, size_t n_totals) {
		device = device_;
		bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
		ev.assign(n_events, nullptr);
		for (hipEvent_t &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
		return ok && !d_tot.alloc(n_totals) && hipMemsetAsync(d_tot.p, 0, n_totals * 8, st) == hipSuccess;
	}
	// the end of a create: its uploads and memsets are through (the host arrays are free again; the counters are zero before a mapper's
	// stream adds to them), or the message
	bool ready(const char *fn, bool ok) {
		ok = ok && hipStreamSynchronize(st) == hipSuccess;
		if (!ok) pipeline_set_error("%s: set-up failed on device %d (%s)", fn, device, hipGetErrorString(hipGetLastError()));
		return ok;
	}
	void close() {
		if (st) (void) hipStreamSynchronize(st);
		for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e);
		if (st) (void) hipStreamDestroy(st);
		st = nullptr; ev.clear();
	}
	// a batch arrives: the lock for as long as lk lives, and after the finish the refusal (the whole message) and -22
	int begin_add(std::unique_lock<std::mutex> &lk, const char *refusal) {
		lk = std::unique_lock<std::mutex>(mu);
		if (finished) { pipeline_set_error("%s", refusal); return -22; }
		return 0;
	}
	// the launch between ev[e0] and ev[e0 + 1]; took() after the caller's synchronise
	template <typename Launch>
	int timed(int e0, Launch launch) {
		NGM_HIP_TRY(hipEventRecord(ev[e0], st));
		launch();
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(hipEventRecord(ev[e0 + 1], st));
		return 0;
	}
	void took(int slot, int e0, int e1) {
		float t = 0.f;
		if (hipEventElapsedTime(&t, ev[e0], ev[e1]) == hipSuccess) ms[slot] += t;
	}
	// the add kernel of a staged batch, through before this returns (the staging buffers are free for the next call), its time into ms[0]
	template <typename Launch>
	int add_kernel(Launch launch) {
		if (int rc = timed(0, launch)) return rc;
		NGM_HIP_TRY(hipStreamSynchronize(st));
		took(0, 0, 1);
		return 0;
	}
	int read_totals(const char *fn, uint64_t *counts, size_t k) const {
		DeviceGuard g(device);
		unsigned long long h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		if (k > 8 || hipMemcpy(h, d_tot.p, k * 8, hipMemcpyDeviceToHost) != hipSuccess) { pipeline_set_error("%s: the counters could not be read (%s)", fn, hipGetErrorString(hipGetLastError())); return -5; }
		for (size_t i = 0; i < k; ++i) counts[i] = h[i];
		return 0;
	}
	// the time an add kernel took on a mapper's stream
	void note_add_ms(float t) {
		std::lock_guard<std::mutex> lk(mu);
		ms[0] += t;
	}
};

// the mapper's SAM stage (mapper_sam.cpp): the device an object lives on, and the time an add kernel on the mapper's stream took
inline int device(const Base *b) { return b ? b->device : -1; }
inline void note_add_ms(Base *b, float t) { if (b) b->note_add_ms(t); }

// ngm_*_destroy: the buffers free themselves while the device is still the object's
template <typename T>
inline void destroy(T *c) {
	if (!c) return;
	DeviceGuard g(c->device);
	c->close();
	delete c;
}

// a batch on the device: the texts' pointers are shifted so that the offsets count from the caller's first byte, as they came
struct Arrays {
	const int32_t *ref_id, *pos0;
	const uint32_t *cigar_off;
	const char *cigar;
	const uint32_t *seq_off;
	const char *seq, *qual;
	const uint8_t *reverse;
	uint32_t n;
};

struct Staged {   // scratch of an add (under the object's lock)
	Buf<int32_t> a_ref, a_pos;
	Buf<uint32_t> a_off, a_soff;
	Buf<char> a_text, a_seq, a_qual;
	Buf<uint8_t> a_rev;

	// seq_off (with seq_text), qual_text and reverse may be null: such an array is not staged and comes back null
	int upload(hipStream_t st, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
			const char *qual_text, const uint8_t *reverse, size_t n, Arrays *A) {
		const size_t t0 = cigar_off[0], tn = cigar_off[n] - t0, s0 = seq_off ? seq_off[0] : 0, sn = seq_off ? seq_off[n] - s0 : 0;
		if (a_ref.grow(n) || a_pos.grow(n) || a_off.grow(n + 1) || a_text.grow(tn + 1) || (seq_off && (a_soff.grow(n + 1) || a_seq.grow(sn + 1))) || (qual_text && a_qual.grow(sn + 1)) ||
				(reverse && a_rev.grow(n))) {
			pipeline_set_error("out of device memory for %zu alignments", n);
			return -12;
		}
		NGM_HIP_TRY(hipMemcpyAsync(a_ref.p, ref_id, n * 4, hipMemcpyHostToDevice, st));
		NGM_HIP_TRY(hipMemcpyAsync(a_pos.p, pos0, n * 4, hipMemcpyHostToDevice, st));
		NGM_HIP_TRY(hipMemcpyAsync(a_off.p, cigar_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
		if (seq_off) NGM_HIP_TRY(hipMemcpyAsync(a_soff.p, seq_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
		if (reverse) NGM_HIP_TRY(hipMemcpyAsync(a_rev.p, reverse, n, hipMemcpyHostToDevice, st));
		if (tn) NGM_HIP_TRY(hipMemcpyAsync(a_text.p, cigar_text + t0, tn, hipMemcpyHostToDevice, st));
		if (sn) NGM_HIP_TRY(hipMemcpyAsync(a_seq.p, seq_text + s0, sn, hipMemcpyHostToDevice, st));
		if (sn && qual_text) NGM_HIP_TRY(hipMemcpyAsync(a_qual.p, qual_text + s0, sn, hipMemcpyHostToDevice, st));
		*A = Arrays{a_ref.p, a_pos.p, a_off.p, a_text.p - t0, seq_off ? a_soff.p : nullptr, seq_off ? a_seq.p - s0 : nullptr, qual_text ? a_qual.p - s0 : nullptr, reverse ? a_rev.p : nullptr, (uint32_t) n};
		return 0;
	}
	void release() { a_ref.release(); a_pos.release(); a_off.release(); a_soff.release(); a_text.release(); a_seq.release(); a_qual.release(); a_rev.release(); }
};

struct Names {   // the contigs' names, concatenated, for the kernels that write lines
	Buf<char> d_names;
	Buf<uint32_t> d_name_off;   // [n_ref + 1]
	bool upload(const RefView &v, hipStream_t st) {   // (the stream is synchronised by the caller before this returns to its caller)
		v.name_table(text, off);
		return put(d_names, text, st) && put(d_name_off, off, st);
	}
private:
	std::vector<char> text;
	std::vector<uint32_t> off;
};

struct Genome {   // the packed reference an object reads: a resident one's, or the caller's own words placed on the object's device
	Buf<uint32_t> own;
	const uint32_t *p = nullptr;
	bool place(const char *fn, const RefView &v, const uint32_t *resident, int device) {
		if (!resident && (own.alloc(v.words.size()) || hipMemcpy(own.p, v.words.data(), v.words.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
			pipeline_set_error("%s: the packed reference (%zu bytes) could not be placed on device %d", fn, v.words.size() * 4, device);
			return false;
		}
		p = resident ? resident : own.p;
		return true;
	}
};

#ifdef NGM_SIDE_LINE_STREAM
struct Widen { __host__ __device__ uint64_t operator()(uint32_t x) const { return (uint64_t) x; } };

// The finish of a per-base text output, chunk by chunk so that the temporaries are bounded whatever the genome's size: the depth by an
// in-place inclusive scan, the object's flag kernel, the flagged slots' chunk offsets by a select (idx[m]); then the object's lengths
// kernel (len[m]), the lines' offsets by a widened exclusive scan, the object's write kernel and the text's download.  Times into the
// object's ms[1] (scan), ms[2] (flags and select), ms[3] (text), between ev[0..4].
struct LineStream {
	Buf<uint8_t> flag, tmp;
	Buf<uint32_t> idx, len, d_m;
	Buf<uint64_t> line_off;
	Buf<char> d_text;
	std::vector<char> text;   // the lines not handed out yet start at text_at
	size_t text_at = 0, chunk = 0;
	uint64_t next_slot = 0;

	static constexpr size_t kDefaultChunk = (size_t) 1 << 25;   // slots scanned at a time: 128 MiB of counters, 160 MiB of temporaries
	static constexpr size_t kMaxChunk = (size_t) 1 << 30;       // (the chunk offsets in idx are 32-bit)
	bool open(size_t scan_chunk) { chunk = std::min(scan_chunk ? scan_chunk : kDefaultChunk, kMaxChunk); return !d_m.alloc(1); }
	// in the finish: the temporaries of a chunk of n slots; refusal is the message for too little memory, with a %zu for n
	int reserve(Base &b, size_t n, const char *refusal) {
		size_t tb = 0, tb2 = 0;
		NGM_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, (int32_t *) nullptr, (int32_t *) nullptr, (int32_t) 0, n, rocprim::plus<int32_t>(), b.st));
		NGM_HIP_TRY(rocprim::select(nullptr, tb2, rocprim::counting_iterator<uint32_t>(0), (uint8_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, n, b.st));
		if (flag.alloc(n) || idx.alloc(n) || tmp.alloc(std::max(tb, tb2) + 16)) { pipeline_set_error(refusal, n); return -12; }
		return 0;
	}
	// the chunk of n slots at depth, the depth in front of it carried in; flag_launch fills flag[n] from the scanned depth.  *m: the
	// flagged slots; *last_depth: the depth behind the chunk.  The chunk's text starts empty and next_slot moves behind the chunk.
	template <typename Launch>
	int scan_and_select(Base &b, int32_t *depth, int32_t carry, size_t n, Launch flag_launch, uint32_t *m, int32_t *last_depth) {
		size_t tb = tmp.cap;
		NGM_HIP_TRY(hipEventRecord(b.ev[0], b.st));
		NGM_HIP_TRY(rocprim::inclusive_scan(tmp.p, tb, depth, depth, carry, n, rocprim::plus<int32_t>(), b.st));
		NGM_HIP_TRY(hipEventRecord(b.ev[1], b.st));
		flag_launch();
		NGM_HIP_TRY(hipGetLastError());
		tb = tmp.cap;
		NGM_HIP_TRY(rocprim::select(tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), flag.p, idx.p, d_m.p, n, b.st));
		NGM_HIP_TRY(hipEventRecord(b.ev[2], b.st));
		NGM_HIP_TRY(hipMemcpyAsync(m, d_m.p, 4, hipMemcpyDeviceToHost, b.st));
		NGM_HIP_TRY(hipMemcpyAsync(last_depth, depth + n - 1, 4, hipMemcpyDeviceToHost, b.st));
		NGM_HIP_TRY(hipStreamSynchronize(b.st));
		b.took(1, 0, 1);
		b.took(2, 1, 2);
		text.clear();
		text_at = 0;
		next_slot += n;
		return 0;
	}
	// The two steps above for an output without a depth array: the temporaries of the select alone, and a chunk of n slots that
	// flag_launch flags from the object's own counters -- no scan.  Times into ms[1] (flags) and ms[2] (select).
	int reserve_select(Base &b, size_t n, const char *refusal) {
		size_t tb = 0;
		NGM_HIP_TRY(rocprim::select(nullptr, tb, rocprim::counting_iterator<uint32_t>(0), (uint8_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, n, b.st));
		if (flag.alloc(n) || idx.alloc(n) || tmp.alloc(tb + 16)) { pipeline_set_error(refusal, n); return -12; }
		return 0;
	}
	template <typename Launch>
	int select_only(Base &b, size_t n, Launch flag_launch, uint32_t *m) {
		NGM_HIP_TRY(hipEventRecord(b.ev[0], b.st));
		flag_launch();
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(hipEventRecord(b.ev[1], b.st));
		size_t tb = tmp.cap;
		NGM_HIP_TRY(rocprim::select(tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), flag.p, idx.p, d_m.p, n, b.st));
		NGM_HIP_TRY(hipEventRecord(b.ev[2], b.st));
		NGM_HIP_TRY(hipMemcpyAsync(m, d_m.p, 4, hipMemcpyDeviceToHost, b.st));
		NGM_HIP_TRY(hipStreamSynchronize(b.st));
		b.took(1, 0, 1);
		b.took(2, 1, 2);
		text.clear();
		text_at = 0;
		next_slot += n;
		return 0;
	}
	// the m lines into text: lengths_launch fills len[m] (len and line_off have room by then), write_launch(out) writes line i at
	// out + line_off[i]; refusal is the message for too little memory, with a %u for m
	template <typename Lengths, typename Write>
	int lines(Base &b, uint32_t m, const char *refusal, Lengths lengths_launch, Write write_launch) {
		if (len.grow((size_t) m + 1) || line_off.grow((size_t) m + 1)) { pipeline_set_error(refusal, m); return -12; }
		NGM_HIP_TRY(hipEventRecord(b.ev[3], b.st));
		NGM_HIP_TRY(hipMemsetAsync(len.p + m, 0, 4, b.st));
		lengths_launch();
		NGM_HIP_TRY(hipGetLastError());
		auto widen = rocprim::make_transform_iterator(len.p, Widen());
		size_t sb = 0;
		NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, sb, widen, line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), b.st));
		if (tmp.grow(sb + 16)) { pipeline_set_error("out of device memory for a scan"); return -12; }
		NGM_HIP_TRY(rocprim::exclusive_scan(tmp.p, sb, widen, line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), b.st));
		uint64_t total = 0;
		NGM_HIP_TRY(hipMemcpyAsync(&total, line_off.p + m, 8, hipMemcpyDeviceToHost, b.st));
		NGM_HIP_TRY(hipStreamSynchronize(b.st));
		if (total) {
			if (d_text.grow((size_t) total)) { pipeline_set_error("out of device memory for %llu bytes of lines", (unsigned long long) total); return -12; }
			write_launch(d_text.p);
			NGM_HIP_TRY(hipGetLastError());
		}
		NGM_HIP_TRY(hipEventRecord(b.ev[4], b.st));
		text.resize((size_t) total);
		if (total) NGM_HIP_TRY(hipMemcpyAsync(text.data(), d_text.p, (size_t) total, hipMemcpyDeviceToHost, b.st));
		NGM_HIP_TRY(hipStreamSynchronize(b.st));
		b.took(3, 3, 4);
		return 0;
	}
	// ngm_*_next behind its checks: more() makes the text of the next chunk (0, or its error) for as long as there is none and slots are
	// left; not_ready is the message where the finish has not reserved
	template <typename More>
	long long next(void *out, size_t cap, uint64_t slots, const char *not_ready, More more) {
		while (text_at >= text.size()) {
			if (next_slot >= slots) return 0;
			if (!flag.p) { pipeline_set_error("%s", not_ready); return -22; }
			if (int rc = more()) return rc;
		}
		size_t taken = 0;
		const long long r = take_whole_lines(text.data() + text_at, text.size() - text_at, out, cap, &taken);
		text_at += taken;
		return r;
	}
};

#endif   // NGM_SIDE_LINE_STREAM

}  // namespace side
}  // namespace ngm
