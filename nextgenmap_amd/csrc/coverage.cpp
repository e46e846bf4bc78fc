// coverage.cpp -- host side of `ngm-hip --coverage` (include/ngm_pipeline.h, ngm_coverage_*): one int32 counter per base of the reference in
// HBM for the whole run, +1 / -1 per covered block from every batch, and at the end of the run the bedGraph text made chunk by chunk -- scan,
// run heads, lines -- so that the temporaries are bounded whatever the genome's size.  Kernels: csrc/coverage_device.h; the host-only parts
// (walk, validator, layout, serialiser): csrc/coverage.h; what it shares with the other side outputs: csrc/side_output.h.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/ngm_pipeline.h"
#define NGM_COV_FINISH_KERNELS
#include "coverage_device.h"
#define NGM_SIDE_LINE_STREAM
#include "side_output.h"

namespace cv = ngm::cov;
namespace side = ngm::side;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

struct ngm_coverage : side::Base {   // d_tot: [0] alignments [1] covered bases [2] runs [3] text bytes
	std::vector<uint64_t> off;       // [n_ref + 1]
	Buf<int32_t> counters;
	Buf<uint64_t> d_off;
	side::Names names;
	side::Staged staged;
	side::LineStream ls;             // its idx: the run heads
	uint64_t open_off = 0;           // the run carried from chunk to chunk
	int32_t open_depth = 0;
};

extern "C" ngm_coverage *ngm_coverage_create(const ngm_coverage_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name))) { ngm::pipeline_set_error("ngm_coverage_create: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_arrays("ngm_coverage_create", p->n_ref, p->ref_len, p->ref_name, nullptr, true, false)) return nullptr;
	if (hipSetDevice(p->device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", p->device); return nullptr; }
	ngm_coverage *c = new ngm_coverage();
	c->n_ref = p->n_ref;
	c->off = cv::contig_offsets(p->ref_len, p->n_ref);
	const uint64_t slots = c->off[p->n_ref];
	if (c->counters.alloc(slots)) {
		ngm::pipeline_set_error("out of device memory for the coverage counters (%llu bytes: 4 per base of the reference, on device %d)", (unsigned long long) slots * 4ull, p->device);
		delete c;
		return nullptr;
	}
	bool ok = c->open(p->device, 5, 4) && c->ls.open(p->scan_chunk) && ngm::put(c->d_off, c->off, c->st) && c->names.upload(ref, c->st);
	ok = ok && hipMemsetAsync(c->counters.p, 0, slots * 4, c->st) == hipSuccess;
	if (!c->ready("ngm_coverage_create", ok)) { ngm_coverage_destroy(c); return nullptr; }
	return c;
}

extern "C" void ngm_coverage_destroy(ngm_coverage *c) { side::destroy(c); }

extern "C" int ngm_coverage_add(ngm_coverage *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_coverage_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	if (int rc = side::check_batch("ngm_coverage_add", cigar_off, cigar_text, nullptr, nullptr, nullptr, n, [&](size_t i, const char *cigar, uint32_t len, uint64_t) {
		const int why = cv::check_alignment(ref_id[i], pos0[i], cigar, len, c->n_ref);
		return why == cv::kOk ? nullptr : cv::why(why);
	})) return rc;
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "ngm_coverage_add: add after ngm_coverage_finish")) return rc;
	DeviceGuard g(c->device);
	side::Arrays A{};
	if (int rc = c->staged.upload(c->st, ref_id, pos0, cigar_off, cigar_text, nullptr, nullptr, nullptr, nullptr, n, &A)) return rc;
	const cv::CovArrays S{A.ref_id, A.pos0, A.cigar_off, A.cigar, A.n};
	return c->add_kernel([&] { hipLaunchKernelGGL(cv::cov_add_kernel<cv::CovArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, c->counters.p, (const uint64_t *) c->d_off.p, c->n_ref, c->d_tot.p); });
}

// the mapper's in-place route (mapper_sam.cpp): where its cov_add_kernel adds
side::Base *ngm::side::base(ngm_coverage *c) { return c; }
int ngm::coverage_target(ngm_coverage *c, cv::Target *t) {
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "a batch for the coverage after ngm_coverage_finish")) return rc;
	*t = cv::Target{c->counters.p, c->d_off.p, c->n_ref, c->d_tot.p};
	return 0;
}

extern "C" int ngm_coverage_finish(ngm_coverage *c) {
	if (!c) { ngm::pipeline_set_error("ngm_coverage_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_coverage_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->staged.release();
	return c->ls.reserve(*c, (size_t) std::min<uint64_t>(c->ls.chunk, c->off[c->n_ref]), "out of device memory for the coverage scan (%zu slots per chunk)");
}

// the next chunk of the array: its runs' lines into c->ls.text
static int scan_chunk(ngm_coverage *c) {
	side::LineStream &ls = c->ls;
	const uint64_t s0 = ls.next_slot;
	const size_t n = (size_t) std::min<uint64_t>(ls.chunk, c->off[c->n_ref] - s0);
	int32_t *depth = c->counters.p + s0;
	uint32_t m = 0, last_head = 0;
	int32_t last_depth = 0;
	if (int rc = ls.scan_and_select(*c, depth, c->open_depth, n, [&] {
		hipLaunchKernelGGL(cv::cov_heads_kernel, dim3(blocks_of(n)), dim3(256), 0, c->st, (const int32_t *) depth, (uint32_t) n, c->open_depth, ls.flag.p);
	}, &m, &last_depth)) return rc;
	if (m == 0) return 0;   // the run that was open in front of the chunk is still open behind it
	cv::TextArgs T{};
	T.depth = depth; T.head = ls.idx.p; T.m = m; T.s0 = s0; T.open_off = c->open_off; T.open_depth = c->open_depth; T.off = c->d_off.p; T.n_ref = c->n_ref;
	T.names = c->names.d_names.p; T.name_off = c->names.d_name_off.p; T.totals = c->d_tot.p + 1;
	NGM_HIP_TRY(hipMemcpyAsync(&last_head, ls.idx.p + (m - 1), 4, hipMemcpyDeviceToHost, c->st));   // (through by the first synchronise of lines())
	if (int rc = ls.lines(*c, m, "out of device memory for the lines of %u runs", [&] { T.len = ls.len.p; T.line_off = ls.line_off.p; hipLaunchKernelGGL(cv::cov_lengths_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); },
			[&](char *out) { T.out = out; hipLaunchKernelGGL(cv::cov_write_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); })) return rc;
	c->open_off = s0 + last_head;
	c->open_depth = last_depth;
	return 0;
}

extern "C" long long ngm_coverage_next(ngm_coverage *c, void *out, size_t out_cap) {
	if (!c) { ngm::pipeline_set_error("ngm_coverage_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->finished) { ngm::pipeline_set_error("ngm_coverage_next: ngm_coverage_finish has not been called"); return -22; }
	DeviceGuard g(c->device);
	return c->ls.next(out, out_cap, c->off[c->n_ref], "ngm_coverage_next: ngm_coverage_finish has not succeeded", [&] { return scan_chunk(c); });
}

extern "C" int ngm_coverage_stats(const ngm_coverage *c, uint64_t counts[4], float ms[4]) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);   // (ms is written under it by add, next and the mappers)
	if (counts) if (int rc = c->read_totals("ngm_coverage_stats", counts, 4)) return rc;
	if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->ms[k];
	return 0;
}
