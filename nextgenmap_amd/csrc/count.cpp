// count.cpp -- host side of `ngm-hip --count` (include/ngm_pipeline.h, ngm_count_*): two uint32 counters per base of the union of the BED
// regions and two uint64 per region in HBM for the whole run, fed by every batch, and at the end of the run one reduce kernel that sums
// every region's counters with the mask applied.  Kernels: csrc/count_device.h; the host-only parts (BED reader, tables, the walk of a
// record, the sums, the serialiser): csrc/count.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ngm_pipeline.h"
#define NGM_COUNT_FINISH_KERNELS
#include "count_device.h"
#include "device_util.h"
#include "refindex.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace ct = ngm::cnt;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

struct ngm_count {
	int device = 0, n_ref = 0, min_qual = ct::kDefaultMinQual;
	std::vector<ct::Region> regions;
	ct::Tables tab;                  // the host's copy: ngm_count_mask finds its slots with it
	std::vector<uint32_t> ref_len;
	std::vector<uint32_t> mask;      // one bit per slot, uploaded by the finish
	uint64_t masked_hit = 0;
	mutable std::mutex mu;           // (ngm_count_stats takes it on a const object)
	hipStream_t st = nullptr;
	hipEvent_t ev[2] = {nullptr, nullptr};
	Buf<uint32_t> cnt, d_mask;
	Buf<unsigned long long> reg, d_tot;   // d_tot: [0] alignments [1] those a region took [2] eligible columns [3] conversions
	Buf<uint32_t> own_genome;        // the packed reference, unless a resident one is used
	const uint32_t *genome = nullptr;
	Buf<uint32_t> d_iv_start, d_iv_end, d_contig_iv, d_rs_start, d_rs_end, d_rs_maxend, d_rs_index, d_contig_rs, d_ref_len, d_rg_len;
	Buf<uint64_t> d_iv_slot, d_start, d_rg_gbase, d_rg_slot0;
	Buf<uint8_t> d_rs_take, d_rg_take;
	Buf<long long> d_out;
	std::vector<long long> out;      // [n_regions][6] after the finish
	bool finished = false, reduced = false;
	// scratch of add (under mu)
	Buf<int32_t> a_ref, a_pos;
	Buf<uint32_t> a_off, a_soff;
	Buf<char> a_text, a_seq, a_qual;
	Buf<uint8_t> a_rev;
	float ms[2] = {0, 0};
};

namespace {
template <typename T> bool put(Buf<T> &b, const std::vector<T> &v, hipStream_t st) {
	return !b.alloc(v.size()) && (v.empty() || hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess);
}

// everything but the packed reference: the regions' tables, the counters
ngm_count *create_common(const ngm_count_params *p, int device, int n_ref, const uint32_t *ref_len, const std::vector<uint64_t> &start) {
	if (p->min_qual < 0 || p->min_qual > 93) { ngm::pipeline_set_error("ngm_count_create: min_qual is not in 0..93"); return nullptr; }
	if (p->n_regions == 0) { ngm::pipeline_set_error("ngm_count_create: no region"); return nullptr; }
	if (p->n_regions > 0x7fffffffu || !p->region_ref || !p->region_start || !p->region_end || !p->region_strand) { ngm::pipeline_set_error("ngm_count_create: bad arguments"); return nullptr; }
	std::vector<ct::Region> regions(p->n_regions);
	for (size_t i = 0; i < p->n_regions; ++i) {
		ct::Region &r = regions[i];
		r.contig = p->region_ref[i]; r.start = p->region_start[i]; r.end = p->region_end[i]; r.strand = p->region_strand[i];
		if (r.contig < 0 || r.contig >= n_ref) { ngm::pipeline_set_error("ngm_count_create: region %zu: its contig is not in [0, n_ref)", i); return nullptr; }
		if (r.start >= r.end) { ngm::pipeline_set_error("ngm_count_create: region %zu: its start is not in front of its end", i); return nullptr; }
		if (r.end > ref_len[r.contig]) { ngm::pipeline_set_error("ngm_count_create: region %zu: its end lies behind the contig's last base", i); return nullptr; }
		if (r.strand != '+' && r.strand != '-' && r.strand != '.') { ngm::pipeline_set_error("ngm_count_create: region %zu: its strand is not +, - or .", i); return nullptr; }
	}
	if (hipSetDevice(device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", device); return nullptr; }
	ngm_count *c = new ngm_count();
	c->device = device; c->n_ref = n_ref; c->min_qual = p->min_qual;
	c->regions.swap(regions);
	c->tab.build(c->regions, n_ref);
	c->ref_len.assign(ref_len, ref_len + n_ref);
	const uint64_t slots = c->tab.slots;
	const size_t n = c->regions.size(), mask_words = (size_t) ((slots + 31) / 32) + 1;
	c->mask.assign(mask_words, 0u);
	if (c->cnt.alloc((size_t) slots * 2) || c->d_mask.alloc(mask_words) || c->reg.alloc(n * 2) || c->d_out.alloc(n * 6)) {
		ngm::pipeline_set_error("out of device memory for the conversion counters (%llu bytes: 8 per base of the regions' union and 64 per region, on device %d)",
				(unsigned long long) slots * 8ull + (unsigned long long) n * 64ull, device);
		delete c;
		return nullptr;
	}
	// what the reduce kernel reads of a region
	const ct::Layout H = c->tab.layout(c->ref_len.data(), nullptr, start.data(), n_ref, c->min_qual);
	std::vector<uint64_t> rg_gbase(n), rg_slot0(n, 0);
	std::vector<uint32_t> rg_len(n);
	std::vector<uint8_t> rg_take(n);
	for (size_t i = 0; i < n; ++i) {
		const ct::Region &r = c->regions[i];
		rg_gbase[i] = start[r.contig] + r.start; rg_len[i] = r.end - r.start; rg_take[i] = ct::take_of(r.strand);
		(void) ct::slot_of(H, r.contig, r.start, &rg_slot0[i]);   // (a region lies inside one interval)
	}
	bool ok = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) == hipSuccess;
	for (hipEvent_t &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	ok = ok && !c->d_tot.alloc(4);
	ok = ok && put(c->d_iv_start, c->tab.iv_start, c->st) && put(c->d_iv_end, c->tab.iv_end, c->st) && put(c->d_iv_slot, c->tab.iv_slot, c->st) && put(c->d_contig_iv, c->tab.contig_iv, c->st);
	ok = ok && put(c->d_rs_start, c->tab.rs_start, c->st) && put(c->d_rs_end, c->tab.rs_end, c->st) && put(c->d_rs_maxend, c->tab.rs_maxend, c->st) && put(c->d_rs_index, c->tab.rs_index, c->st);
	ok = ok && put(c->d_rs_take, c->tab.rs_take, c->st) && put(c->d_contig_rs, c->tab.contig_rs, c->st) && put(c->d_ref_len, c->ref_len, c->st) && put(c->d_start, start, c->st);
	ok = ok && put(c->d_rg_gbase, rg_gbase, c->st) && put(c->d_rg_slot0, rg_slot0, c->st) && put(c->d_rg_len, rg_len, c->st) && put(c->d_rg_take, rg_take, c->st);
	ok = ok && hipMemsetAsync(c->cnt.p, 0, std::max<size_t>((size_t) slots * 8, 4), c->st) == hipSuccess && hipMemsetAsync(c->reg.p, 0, n * 16, c->st) == hipSuccess;
	ok = ok && hipMemsetAsync(c->d_tot.p, 0, 32, c->st) == hipSuccess && hipMemsetAsync(c->d_out.p, 0, n * 48, c->st) == hipSuccess;
	ok = ok && hipStreamSynchronize(c->st) == hipSuccess;   // (the host arrays are free again; the counters are zero before a mapper's stream adds to them)
	if (!ok) { ngm::pipeline_set_error("ngm_count_create: set-up failed on device %d (%s)", device, hipGetErrorString(hipGetLastError())); ngm_count_destroy(c); return nullptr; }
	return c;
}

ct::Layout layout_of(const ngm_count *c) {
	return ct::Layout{c->d_iv_start.p, c->d_iv_end.p, c->d_iv_slot.p, c->d_contig_iv.p, c->d_rs_start.p, c->d_rs_end.p, c->d_rs_maxend.p, c->d_rs_index.p, c->d_rs_take.p, c->d_contig_rs.p,
			c->d_ref_len.p, c->genome, c->d_start.p, c->n_ref, c->min_qual};
}
ct::Counters counters_of(const ngm_count *c) { return ct::Counters{c->cnt.p, c->reg.p, c->d_tot.p}; }
}  // namespace

extern "C" ngm_count *ngm_count_create(const ngm_count_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name || !p->ref_seq))) { ngm::pipeline_set_error("ngm_count_create: bad arguments"); return nullptr; }
	for (int c = 0; c < p->n_ref; ++c) {
		if (!p->ref_seq[c] || strnlen(p->ref_seq[c], (size_t) p->ref_len[c]) != (size_t) p->ref_len[c]) { ngm::pipeline_set_error("ngm_count_create: the sequence of contig %d is shorter than its length", c); return nullptr; }
	}
	std::vector<uint64_t> start;
	const std::vector<uint32_t> words = sn::pack_reference(p->ref_seq, p->ref_len, p->n_ref, start);
	ngm_count *c = create_common(p, p->device, p->n_ref, p->ref_len, start);
	if (!c) return nullptr;
	if (c->own_genome.alloc(words.size()) || hipMemcpy(c->own_genome.p, words.data(), words.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
		ngm::pipeline_set_error("ngm_count_create: the packed reference (%zu bytes) could not be placed on device %d", words.size() * 4, p->device);
		ngm_count_destroy(c);
		return nullptr;
	}
	c->genome = c->own_genome.p;
	return c;
}

extern "C" ngm_count *ngm_count_create_for_ref(const ngm_ref *r, const ngm_count_params *p) {
	if (!r || !p || !r->d_genome) { ngm::pipeline_set_error("ngm_count_create_for_ref: bad arguments"); return nullptr; }
	const int n_ref = (int) r->contigs.size();
	std::vector<uint32_t> lens((size_t) n_ref);
	std::vector<uint64_t> start((size_t) n_ref + 1, 0);
	for (int c = 0; c < n_ref; ++c) {
		if (r->contigs[c].len > 0xffffffffull || r->contigs[c].start + r->contigs[c].len > r->genome_words * 8ull) { ngm::pipeline_set_error("ngm_count_create_for_ref: contig %d does not fit", c); return nullptr; }
		lens[c] = (uint32_t) r->contigs[c].len; start[c] = r->contigs[c].start;
	}
	start[n_ref] = r->genome_words * 8ull;
	ngm_count *c = create_common(p, r->device, n_ref, lens.data(), start);
	if (c) c->genome = r->d_genome;   // (the reference outlives the run's caller)
	return c;
}

extern "C" void ngm_count_destroy(ngm_count *c) {
	if (!c) return;
	DeviceGuard g(c->device);
	if (c->st) (void) hipStreamSynchronize(c->st);
	for (hipEvent_t e : c->ev) if (e) (void) hipEventDestroy(e);
	if (c->st) (void) hipStreamDestroy(c->st);
	delete c;   // (the buffers free themselves: the device is still this one)
}

extern "C" int ngm_count_add(ngm_count *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
		const char *qual_text, const uint8_t *reverse, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off || !seq_off || !reverse)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_count_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	// the checks of ngm_snp_add: over the caller's memory, before anything of it reaches the device
	const size_t qual_len = qual_text ? strlen(qual_text) : 0;
	for (size_t i = 0; i < n; ++i) {
		if (cigar_off[i + 1] < cigar_off[i] || (cigar_off[i + 1] > cigar_off[i] && !cigar_text)) { ngm::pipeline_set_error("ngm_count_add: alignment %zu: its CIGAR offsets do not ascend", i); return -22; }
		if (seq_off[i + 1] < seq_off[i] || (seq_off[i + 1] > seq_off[i] && !seq_text)) { ngm::pipeline_set_error("ngm_count_add: alignment %zu: its sequence offsets do not ascend", i); return -22; }
		const int why = sn::check_alignment(ref_id[i], pos0[i], cigar_text + cigar_off[i], cigar_off[i + 1] - cigar_off[i], c->n_ref, (uint64_t) (seq_off[i + 1] - seq_off[i]));
		if (why != cv::kOk) { ngm::pipeline_set_error("ngm_count_add: alignment %zu: %s", i, sn::why(why)); return -22; }
		if (qual_text && (size_t) seq_off[i + 1] > qual_len) { ngm::pipeline_set_error("ngm_count_add: alignment %zu: %s", i, sn::why(sn::kQualLength)); return -22; }
	}
	if (qual_text && qual_len != (size_t) seq_off[n]) { ngm::pipeline_set_error("ngm_count_add: alignment %zu: %s", n - 1, sn::why(sn::kQualLength)); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_count_add: add after ngm_count_finish"); return -22; }
	DeviceGuard g(c->device);
	const size_t t0 = cigar_off[0], tn = cigar_off[n] - t0, s0 = seq_off[0], sn_bytes = seq_off[n] - s0;
	if (c->a_ref.grow(n) || c->a_pos.grow(n) || c->a_off.grow(n + 1) || c->a_soff.grow(n + 1) || c->a_rev.grow(n) || c->a_text.grow(tn + 1) || c->a_seq.grow(sn_bytes + 1) ||
			(qual_text && c->a_qual.grow(sn_bytes + 1))) {
		ngm::pipeline_set_error("out of device memory for %zu alignments", n);
		return -12;
	}
	NGM_HIP_TRY(hipMemcpyAsync(c->a_ref.p, ref_id, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_pos.p, pos0, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_off.p, cigar_off, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_soff.p, seq_off, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_rev.p, reverse, n, hipMemcpyHostToDevice, c->st));
	if (tn) NGM_HIP_TRY(hipMemcpyAsync(c->a_text.p, cigar_text + t0, tn, hipMemcpyHostToDevice, c->st));
	if (sn_bytes) NGM_HIP_TRY(hipMemcpyAsync(c->a_seq.p, seq_text + s0, sn_bytes, hipMemcpyHostToDevice, c->st));
	if (sn_bytes && qual_text) NGM_HIP_TRY(hipMemcpyAsync(c->a_qual.p, qual_text + s0, sn_bytes, hipMemcpyHostToDevice, c->st));
	// (the offsets count from the caller's first byte)
	const ct::CountArrays S{sn::SnpArrays{c->a_ref.p, c->a_pos.p, c->a_off.p, c->a_text.p - t0, c->a_soff.p, c->a_seq.p - s0, qual_text ? c->a_qual.p - s0 : nullptr, (uint32_t) n}, c->a_rev.p};
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	hipLaunchKernelGGL(ct::count_add_kernel<ct::CountArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, layout_of(c), counters_of(c));
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	float t = 0.f;
	if (hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[0] += t;
	return 0;
}

// the mapper's in-place route (mapper.cpp): where its count_add_kernel adds, and the time that kernel took
int ngm::count_device(const ngm_count *c) { return c ? c->device : -1; }
int ngm::count_target(ngm_count *c, ngm::cnt::Layout *l, ngm::cnt::Counters *t) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("a batch for the conversion counters after ngm_count_finish"); return -22; }
	*l = layout_of(c);
	*t = counters_of(c);
	return 0;
}
void ngm::count_note_add_ms(ngm_count *c, float ms) {
	if (!c) return;
	std::lock_guard<std::mutex> lk(c->mu);
	c->ms[0] += ms;
}

extern "C" int ngm_count_mask(ngm_count *c, const int32_t *ref_id, const int32_t *pos0, size_t n) {
	if (!c || (n && (!ref_id || !pos0))) { ngm::pipeline_set_error("ngm_count_mask: bad arguments"); return -22; }
	for (size_t i = 0; i < n; ++i) {
		if (ref_id[i] < 0 || ref_id[i] >= c->n_ref) { ngm::pipeline_set_error("ngm_count_mask: position %zu: its ref_id is not in [0, n_ref)", i); return -22; }
		if (pos0[i] < 0 || (uint32_t) pos0[i] >= c->ref_len[(size_t) ref_id[i]]) { ngm::pipeline_set_error("ngm_count_mask: position %zu: it is not inside its contig", i); return -22; }
	}
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_count_mask: called after ngm_count_finish"); return -22; }
	const ct::Layout H = c->tab.layout(c->ref_len.data(), nullptr, nullptr, c->n_ref, c->min_qual);
	for (size_t i = 0; i < n; ++i) {
		uint64_t slot = 0;
		if (!ct::slot_of(H, ref_id[i], (uint32_t) pos0[i], &slot) || ct::mask_bit(c->mask.data(), slot)) continue;   // (outside every region, or masked already)
		c->mask[(size_t) (slot >> 5)] |= 1u << (uint32_t) (slot & 31u);
		++c->masked_hit;
	}
	return 0;
}

extern "C" int ngm_count_finish(ngm_count *c) {
	if (!c) { ngm::pipeline_set_error("ngm_count_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_count_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->a_ref.release(); c->a_pos.release(); c->a_off.release(); c->a_soff.release(); c->a_text.release(); c->a_seq.release(); c->a_qual.release(); c->a_rev.release();
	const size_t n = c->regions.size();
	NGM_HIP_TRY(hipMemcpyAsync(c->d_mask.p, c->mask.data(), c->mask.size() * 4, hipMemcpyHostToDevice, c->st));
	ct::ReduceArgs A{c->d_rg_gbase.p, c->d_rg_slot0.p, c->d_rg_len.p, c->d_rg_take.p, (uint32_t) n, c->genome, c->cnt.p, c->d_mask.p, c->reg.p, c->d_out.p};
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	hipLaunchKernelGGL(ct::count_reduce_kernel, dim3((unsigned) ((n + 3) / 4)), dim3(256), 0, c->st, A);   // (four waves, four regions, per block)
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	c->out.assign(n * 6, 0);
	NGM_HIP_TRY(hipMemcpyAsync(c->out.data(), c->d_out.p, n * 48, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	float t = 0.f;
	if (hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[1] += t;
	c->reduced = true;
	return 0;
}

extern "C" long long ngm_count_read(ngm_count *c, int64_t *out, size_t n_regions) {
	if (!c) { ngm::pipeline_set_error("ngm_count_read: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->reduced) { ngm::pipeline_set_error("ngm_count_read: ngm_count_finish has not succeeded"); return -22; }
	if (!out) return (long long) c->regions.size();
	if (n_regions != c->regions.size()) { ngm::pipeline_set_error("ngm_count_read: the object has %zu regions, not %zu", c->regions.size(), n_regions); return -22; }
	for (size_t i = 0; i < c->out.size(); ++i) out[i] = (int64_t) c->out[i];
	return (long long) c->regions.size();
}

extern "C" int ngm_count_stats(const ngm_count *c, uint64_t counts[5], float ms[2]) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);   // (masked_hit and ms are written under it by mask, add and the mappers)
	if (counts) {
		DeviceGuard g(c->device);
		unsigned long long h[4] = {0, 0, 0, 0};
		if (hipMemcpy(h, c->d_tot.p, 32, hipMemcpyDeviceToHost) != hipSuccess) { ngm::pipeline_set_error("ngm_count_stats: the counters could not be read (%s)", hipGetErrorString(hipGetLastError())); return -5; }
		for (int k = 0; k < 4; ++k) counts[k] = h[k];
		counts[4] = c->masked_hit;
	}
	if (ms) for (int k = 0; k < 2; ++k) ms[k] = c->ms[k];
	return 0;
}
