// coverage.cpp -- host side of `ngm-hip --coverage` (include/ngm_pipeline.h, ngm_coverage_*): one int32 counter per base of the reference in
// HBM for the whole run, +1 / -1 per covered block from every batch, and at the end of the run the bedGraph text made chunk by chunk -- scan,
// run heads, lines -- so that the temporaries are bounded whatever the genome's size.  Kernels: csrc/coverage_device.h; the host-only parts
// (walk, validator, layout, serialiser): csrc/coverage.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>   // (after <cstring>: its texture iterator calls the host's memset)

#include "../../include/ngm_pipeline.h"
#define NGM_COV_FINISH_KERNELS
#include "coverage_device.h"
#include "device_util.h"
#include "refindex.h"

namespace cv = ngm::cov;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

namespace {
constexpr size_t kDefaultChunk = (size_t) 1 << 25;   // slots scanned at a time: 128 MiB of counters, 160 MiB of temporaries
constexpr size_t kMaxChunk = (size_t) 1 << 30;       // (the heads' chunk offsets are 32-bit)
}  // namespace

struct ngm_coverage {
	int device = 0, n_ref = 0;
	size_t chunk = kDefaultChunk;
	std::vector<uint64_t> off;      // [n_ref + 1]
	std::mutex mu;
	hipStream_t st = nullptr;
	hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	Buf<int32_t> counters;
	Buf<uint64_t> d_off;
	Buf<char> d_names;
	Buf<uint32_t> d_name_off;
	Buf<unsigned long long> d_tot;  // [0] alignments [1] covered bases [2] runs [3] text bytes
	bool finished = false;
	// scratch of add (under mu)
	Buf<int32_t> a_ref, a_pos;
	Buf<uint32_t> a_off;
	Buf<char> a_text;
	// the finish: temporaries of a chunk, the run carried from chunk to chunk, the chunk's text on the host
	Buf<uint8_t> flag, tmp;
	Buf<uint32_t> head, len, d_m;
	Buf<uint64_t> line_off;
	Buf<char> d_text;
	uint64_t next_slot = 0, open_off = 0;
	int32_t open_depth = 0;
	std::vector<char> text;
	size_t text_at = 0;
	float ms[4] = {0, 0, 0, 0};
};

extern "C" ngm_coverage *ngm_coverage_create(const ngm_coverage_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name))) { ngm::pipeline_set_error("ngm_coverage_create: bad arguments"); return nullptr; }
	for (int c = 0; c < p->n_ref; ++c) if (!p->ref_name[c]) { ngm::pipeline_set_error("ngm_coverage_create: contig %d has no name", c); return nullptr; }
	if (hipSetDevice(p->device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", p->device); return nullptr; }
	ngm_coverage *c = new ngm_coverage();
	c->device = p->device;
	c->n_ref = p->n_ref;
	c->chunk = std::min(p->scan_chunk ? p->scan_chunk : kDefaultChunk, kMaxChunk);
	c->off = cv::contig_offsets(p->ref_len, p->n_ref);
	const uint64_t slots = c->off[p->n_ref];
	std::string names;
	std::vector<uint32_t> name_off((size_t) p->n_ref + 1, 0);
	for (int k = 0; k < p->n_ref; ++k) { names += p->ref_name[k]; name_off[(size_t) k + 1] = (uint32_t) names.size(); }
	if (c->counters.alloc(slots)) {
		ngm::pipeline_set_error("out of device memory for the coverage counters (%llu bytes: 4 per base of the reference, on device %d)", (unsigned long long) slots * 4ull, p->device);
		delete c;
		return nullptr;
	}
	bool ok = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) == hipSuccess;
	for (hipEvent_t &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	ok = ok && !c->d_off.alloc(c->off.size()) && !c->d_names.alloc(names.size()) && !c->d_name_off.alloc(name_off.size()) && !c->d_tot.alloc(4) && !c->d_m.alloc(1);
	ok = ok && hipMemsetAsync(c->counters.p, 0, slots * 4, c->st) == hipSuccess && hipMemsetAsync(c->d_tot.p, 0, 32, c->st) == hipSuccess;
	ok = ok && hipMemcpyAsync(c->d_off.p, c->off.data(), c->off.size() * 8, hipMemcpyHostToDevice, c->st) == hipSuccess;
	ok = ok && (names.empty() || hipMemcpyAsync(c->d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->st) == hipSuccess);
	ok = ok && hipMemcpyAsync(c->d_name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, c->st) == hipSuccess;
	ok = ok && hipStreamSynchronize(c->st) == hipSuccess;   // (the host arrays are free again; the counters are zero before a mapper's stream adds to them)
	if (!ok) { ngm::pipeline_set_error("ngm_coverage_create: set-up failed on device %d (%s)", p->device, hipGetErrorString(hipGetLastError())); ngm_coverage_destroy(c); return nullptr; }
	return c;
}

extern "C" void ngm_coverage_destroy(ngm_coverage *c) {
	if (!c) return;
	DeviceGuard g(c->device);
	if (c->st) (void) hipStreamSynchronize(c->st);
	for (hipEvent_t e : c->ev) if (e) (void) hipEventDestroy(e);
	if (c->st) (void) hipStreamDestroy(c->st);
	delete c;   // (the buffers free themselves: the device is still this one)
}

extern "C" int ngm_coverage_add(ngm_coverage *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_coverage_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	// the checks need no lock: they are over the caller's memory, before anything of it reaches the device
	for (size_t i = 0; i < n; ++i) {
		if (cigar_off[i + 1] < cigar_off[i] || (cigar_off[i + 1] > cigar_off[i] && !cigar_text)) { ngm::pipeline_set_error("ngm_coverage_add: alignment %zu: its CIGAR offsets do not ascend", i); return -22; }
		const int why = cv::check_alignment(ref_id[i], pos0[i], cigar_text + cigar_off[i], cigar_off[i + 1] - cigar_off[i], c->n_ref);
		if (why != cv::kOk) { ngm::pipeline_set_error("ngm_coverage_add: alignment %zu: %s", i, cv::why(why)); return -22; }
	}
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_coverage_add: add after ngm_coverage_finish"); return -22; }
	DeviceGuard g(c->device);
	const size_t t0 = cigar_off[0], tn = cigar_off[n] - t0;
	if (c->a_ref.grow(n) || c->a_pos.grow(n) || c->a_off.grow(n + 1) || c->a_text.grow(tn + 1)) { ngm::pipeline_set_error("out of device memory for %zu alignments", n); return -12; }
	NGM_HIP_TRY(hipMemcpyAsync(c->a_ref.p, ref_id, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_pos.p, pos0, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_off.p, cigar_off, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
	if (tn) NGM_HIP_TRY(hipMemcpyAsync(c->a_text.p, cigar_text + t0, tn, hipMemcpyHostToDevice, c->st));
	cv::CovArrays S{c->a_ref.p, c->a_pos.p, c->a_off.p, c->a_text.p - t0, (uint32_t) n};   // (the offsets count from the caller's first byte)
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	hipLaunchKernelGGL(cv::cov_add_kernel<cv::CovArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, c->counters.p, (const uint64_t *) c->d_off.p, c->n_ref, c->d_tot.p);
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	float t = 0.f;
	if (hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[0] += t;
	return 0;
}

// the mapper's in-place route (mapper.cpp): where its cov_add_kernel adds, and the time that kernel took
int ngm::coverage_device(const ngm_coverage *c) { return c ? c->device : -1; }
int ngm::coverage_target(ngm_coverage *c, int32_t **counters, const uint64_t **d_off, int *n_ref, unsigned long long **d_n_aln) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("a batch for the coverage after ngm_coverage_finish"); return -22; }
	*counters = c->counters.p; *d_off = c->d_off.p; *n_ref = c->n_ref; *d_n_aln = c->d_tot.p;
	return 0;
}
void ngm::coverage_note_add_ms(ngm_coverage *c, float ms) {
	if (!c) return;
	std::lock_guard<std::mutex> lk(c->mu);
	c->ms[0] += ms;
}

extern "C" int ngm_coverage_finish(ngm_coverage *c) {
	if (!c) { ngm::pipeline_set_error("ngm_coverage_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_coverage_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->a_ref.release(); c->a_pos.release(); c->a_off.release(); c->a_text.release();
	const size_t n = (size_t) std::min<uint64_t>(c->chunk, c->off[c->n_ref]);
	size_t tb = 0, tb2 = 0;
	NGM_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, (int32_t *) nullptr, (int32_t *) nullptr, (int32_t) 0, n, rocprim::plus<int32_t>(), c->st));
	NGM_HIP_TRY(rocprim::select(nullptr, tb2, rocprim::counting_iterator<uint32_t>(0), (uint8_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, n, c->st));
	if (c->flag.alloc(n) || c->head.alloc(n) || c->tmp.alloc(std::max(tb, tb2) + 16)) { ngm::pipeline_set_error("out of device memory for the coverage scan (%zu slots per chunk)", n); return -12; }
	return 0;
}

namespace {
// the next chunk of the array: its runs' lines into c->text
int scan_chunk(ngm_coverage *c) {
	const uint64_t s0 = c->next_slot;
	const size_t n = (size_t) std::min<uint64_t>(c->chunk, c->off[c->n_ref] - s0);
	int32_t *depth = c->counters.p + s0;
	size_t tb = c->tmp.n;
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	NGM_HIP_TRY(rocprim::inclusive_scan(c->tmp.p, tb, depth, depth, c->open_depth, n, rocprim::plus<int32_t>(), c->st));   // (in place, the depth in front carried in)
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	hipLaunchKernelGGL(cv::cov_heads_kernel, dim3(blocks_of(n)), dim3(256), 0, c->st, (const int32_t *) depth, (uint32_t) n, c->open_depth, c->flag.p);
	NGM_HIP_TRY(hipGetLastError());
	tb = c->tmp.n;
	NGM_HIP_TRY(rocprim::select(c->tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), c->flag.p, c->head.p, c->d_m.p, n, c->st));
	NGM_HIP_TRY(hipEventRecord(c->ev[2], c->st));
	uint32_t m = 0;
	int32_t last_depth = 0;
	NGM_HIP_TRY(hipMemcpyAsync(&m, c->d_m.p, 4, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(&last_depth, depth + n - 1, 4, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	float t = 0.f;
	if (hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[1] += t;
	if (hipEventElapsedTime(&t, c->ev[1], c->ev[2]) == hipSuccess) c->ms[2] += t;
	c->text.clear();
	c->text_at = 0;
	c->next_slot = s0 + n;
	if (m == 0) return 0;   // the run that was open in front of the chunk is still open behind it
	if (c->len.grow((size_t) m + 1) || c->line_off.grow((size_t) m + 1)) { ngm::pipeline_set_error("out of device memory for the lines of %u runs", m); return -12; }
	cv::TextArgs T{};
	T.depth = depth; T.head = c->head.p; T.m = m; T.s0 = s0; T.open_off = c->open_off; T.open_depth = c->open_depth; T.off = c->d_off.p; T.n_ref = c->n_ref;
	T.names = c->d_names.p; T.name_off = c->d_name_off.p; T.len = c->len.p; T.line_off = c->line_off.p; T.totals = c->d_tot.p + 1;
	NGM_HIP_TRY(hipEventRecord(c->ev[3], c->st));
	NGM_HIP_TRY(hipMemsetAsync(c->len.p + m, 0, 4, c->st));
	hipLaunchKernelGGL(cv::cov_lengths_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T);
	NGM_HIP_TRY(hipGetLastError());
	auto widen = rocprim::make_transform_iterator(c->len.p, [] __host__ __device__ (uint32_t x) { return (uint64_t) x; });
	size_t sb = 0;
	NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, sb, widen, c->line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), c->st));
	if (c->tmp.grow(sb + 16)) { ngm::pipeline_set_error("out of device memory for a scan"); return -12; }
	NGM_HIP_TRY(rocprim::exclusive_scan(c->tmp.p, sb, widen, c->line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), c->st));
	uint64_t total = 0;
	uint32_t last_head = 0;
	NGM_HIP_TRY(hipMemcpyAsync(&total, c->line_off.p + m, 8, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(&last_head, c->head.p + (m - 1), 4, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	if (total) {
		if (c->d_text.grow((size_t) total)) { ngm::pipeline_set_error("out of device memory for %llu bytes of lines", (unsigned long long) total); return -12; }
		T.out = c->d_text.p;
		hipLaunchKernelGGL(cv::cov_write_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T);
		NGM_HIP_TRY(hipGetLastError());
	}
	NGM_HIP_TRY(hipEventRecord(c->ev[4], c->st));
	c->text.resize((size_t) total);
	if (total) NGM_HIP_TRY(hipMemcpyAsync(c->text.data(), c->d_text.p, (size_t) total, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	if (hipEventElapsedTime(&t, c->ev[3], c->ev[4]) == hipSuccess) c->ms[3] += t;
	c->open_off = s0 + last_head;
	c->open_depth = last_depth;
	return 0;
}
}  // namespace

extern "C" long long ngm_coverage_next(ngm_coverage *c, void *out, size_t out_cap) {
	if (!c) { ngm::pipeline_set_error("ngm_coverage_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->finished) { ngm::pipeline_set_error("ngm_coverage_next: ngm_coverage_finish has not been called"); return -22; }
	DeviceGuard g(c->device);
	while (c->text_at >= c->text.size()) {
		if (c->next_slot >= c->off[c->n_ref]) return 0;
		if (!c->flag.p) { ngm::pipeline_set_error("ngm_coverage_next: ngm_coverage_finish has not succeeded"); return -22; }
		if (int rc = scan_chunk(c)) return rc;
	}
	// whole lines only: as many as fit, or the size of the first one
	const char *p = c->text.data() + c->text_at;
	const size_t left = c->text.size() - c->text_at;
	size_t take = std::min(left, out_cap);
	while (take > 0 && p[take - 1] != '\n') --take;
	if (take == 0 || !out) return (long long) ((const char *) memchr(p, '\n', left) - p + 1);
	memcpy(out, p, take);
	c->text_at += take;
	return (long long) take;
}

extern "C" int ngm_coverage_stats(const ngm_coverage *c, uint64_t counts[4], float ms[4]) {
	if (!c) return -22;
	if (counts) {
		DeviceGuard g(c->device);
		unsigned long long h[4] = {0, 0, 0, 0};
		if (hipMemcpy(h, c->d_tot.p, 32, hipMemcpyDeviceToHost) != hipSuccess) { ngm::pipeline_set_error("ngm_coverage_stats: the counters could not be read (%s)", hipGetErrorString(hipGetLastError())); return -5; }
		for (int k = 0; k < 4; ++k) counts[k] = h[k];
	}
	if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->ms[k];
	return 0;
}
