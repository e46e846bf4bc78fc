// count.cpp -- host side of `ngm-hip --count` (include/ngm_pipeline.h, ngm_count_*): two uint32 counters per base of the union of the BED
// regions and two uint64 per region in HBM for the whole run, fed by every batch, and at the end of the run one reduce kernel that sums
// every region's counters with the mask applied.  Kernels: csrc/count_device.h; the host-only parts (BED reader, tables, the walk of a
// record, the sums, the serialiser): csrc/count.h; what it shares with the other side outputs: csrc/side_output.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ngm_pipeline.h"
#define NGM_COUNT_FINISH_KERNELS
#include "count_device.h"
#include "side_output.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace ct = ngm::cnt;
namespace side = ngm::side;
using ngm::put;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

struct ngm_count : side::Base {   // d_tot: [0] alignments [1] those a region took [2] eligible columns [3] conversions; ms: [0] add [1] reduce
	int min_qual = ct::kDefaultMinQual;
	std::vector<ct::Region> regions;
	ct::Tables tab;                  // the host's copy: ngm_count_mask finds its slots with it
	std::vector<uint32_t> ref_len;
	std::vector<uint32_t> mask;      // one bit per slot, uploaded by the finish
	uint64_t masked_hit = 0;
	Buf<uint32_t> cnt, d_mask;
	Buf<unsigned long long> reg;
	side::Genome genome;
	Buf<uint32_t> d_iv_start, d_iv_end, d_contig_iv, d_rs_start, d_rs_end, d_rs_maxend, d_rs_index, d_contig_rs, d_ref_len, d_rg_len;
	Buf<uint64_t> d_iv_slot, d_start, d_rg_gbase, d_rg_slot0;
	Buf<uint8_t> d_rs_take, d_rg_take;
	Buf<long long> d_out;
	std::vector<long long> out;      // [n_regions][6] after the finish
	bool reduced = false;
	side::Staged staged;
};

namespace {
// the object over the contigs of ref; genome: a resident reference's, or null and ref's own packed words go up
ngm_count *create(const ngm_count_params *p, int device, const side::RefView &ref, const uint32_t *genome) {
	const int n_ref = ref.n_ref();
	const std::vector<uint32_t> &ref_len = ref.lens;
	const std::vector<uint64_t> &start = ref.start;
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
	c->n_ref = n_ref; c->min_qual = p->min_qual;
	c->regions.swap(regions);
	c->tab.build(c->regions, n_ref);
	c->ref_len = ref_len;
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
	bool ok = c->open(device, 2, 4);
	ok = ok && put(c->d_iv_start, c->tab.iv_start, c->st) && put(c->d_iv_end, c->tab.iv_end, c->st) && put(c->d_iv_slot, c->tab.iv_slot, c->st) && put(c->d_contig_iv, c->tab.contig_iv, c->st);
	ok = ok && put(c->d_rs_start, c->tab.rs_start, c->st) && put(c->d_rs_end, c->tab.rs_end, c->st) && put(c->d_rs_maxend, c->tab.rs_maxend, c->st) && put(c->d_rs_index, c->tab.rs_index, c->st);
	ok = ok && put(c->d_rs_take, c->tab.rs_take, c->st) && put(c->d_contig_rs, c->tab.contig_rs, c->st) && put(c->d_ref_len, c->ref_len, c->st) && put(c->d_start, start, c->st);
	ok = ok && put(c->d_rg_gbase, rg_gbase, c->st) && put(c->d_rg_slot0, rg_slot0, c->st) && put(c->d_rg_len, rg_len, c->st) && put(c->d_rg_take, rg_take, c->st);
	ok = ok && hipMemsetAsync(c->cnt.p, 0, std::max<size_t>((size_t) slots * 8, 4), c->st) == hipSuccess && hipMemsetAsync(c->reg.p, 0, n * 16, c->st) == hipSuccess;
	ok = ok && hipMemsetAsync(c->d_out.p, 0, n * 48, c->st) == hipSuccess;
	if (!c->ready("ngm_count_create", ok)) { ngm_count_destroy(c); return nullptr; }
	if (!c->genome.place("ngm_count_create", ref, genome, device)) { ngm_count_destroy(c); return nullptr; }
	return c;
}

ct::Layout layout_of(const ngm_count *c) {
	return ct::Layout{c->d_iv_start.p, c->d_iv_end.p, c->d_iv_slot.p, c->d_contig_iv.p, c->d_rs_start.p, c->d_rs_end.p, c->d_rs_maxend.p, c->d_rs_index.p, c->d_rs_take.p, c->d_contig_rs.p,
			c->d_ref_len.p, c->genome.p, c->d_start.p, c->n_ref, c->min_qual};
}
ct::Counters counters_of(const ngm_count *c) { return ct::Counters{c->cnt.p, c->reg.p, c->d_tot.p}; }
}  // namespace

extern "C" ngm_count *ngm_count_create(const ngm_count_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name || !p->ref_seq))) { ngm::pipeline_set_error("ngm_count_create: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_arrays("ngm_count_create", p->n_ref, p->ref_len, p->ref_name, p->ref_seq, false, true)) return nullptr;
	return create(p, p->device, ref, nullptr);
}

extern "C" ngm_count *ngm_count_create_for_ref(const ngm_ref *r, const ngm_count_params *p) {
	if (!r || !p || !r->d_genome.p) { ngm::pipeline_set_error("ngm_count_create_for_ref: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_ref("ngm_count_create_for_ref", *r)) return nullptr;
	return create(p, r->device, ref, r->d_genome.p);   // (the reference outlives the run's caller)
}

extern "C" void ngm_count_destroy(ngm_count *c) { side::destroy(c); }

extern "C" int ngm_count_add(ngm_count *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
		const char *qual_text, const uint8_t *reverse, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off || !seq_off || !reverse)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_count_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	if (int rc = side::check_batch("ngm_count_add", cigar_off, cigar_text, seq_off, seq_text, qual_text, n, [&](size_t i, const char *cigar, uint32_t len, uint64_t seq_len) {   // (the checks of ngm_snp_add)
		const int why = sn::check_alignment(ref_id[i], pos0[i], cigar, len, c->n_ref, seq_len);
		return why == cv::kOk ? nullptr : sn::why(why);
	})) return rc;
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "ngm_count_add: add after ngm_count_finish")) return rc;
	DeviceGuard g(c->device);
	side::Arrays A{};
	if (int rc = c->staged.upload(c->st, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text, reverse, n, &A)) return rc;
	const ct::CountArrays S{sn::SnpArrays{A.ref_id, A.pos0, A.cigar_off, A.cigar, A.seq_off, A.seq, A.qual, A.n}, A.reverse};
	return c->add_kernel([&] { hipLaunchKernelGGL(ct::count_add_kernel<ct::CountArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, layout_of(c), counters_of(c)); });
}

// the mapper's in-place route (mapper_sam.cpp): the tables and counters its count_add_kernel works with
side::Base *ngm::side::base(ngm_count *c) { return c; }
int ngm::count_target(ngm_count *c, ngm::cnt::Layout *l, ngm::cnt::Counters *t) {
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "a batch for the conversion counters after ngm_count_finish")) return rc;
	*l = layout_of(c);
	*t = counters_of(c);
	return 0;
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
	c->staged.release();
	const size_t n = c->regions.size();
	NGM_HIP_TRY(hipMemcpyAsync(c->d_mask.p, c->mask.data(), c->mask.size() * 4, hipMemcpyHostToDevice, c->st));
	ct::ReduceArgs A{c->d_rg_gbase.p, c->d_rg_slot0.p, c->d_rg_len.p, c->d_rg_take.p, (uint32_t) n, c->genome.p, c->cnt.p, c->d_mask.p, c->reg.p, c->d_out.p};
	if (int rc = c->timed(0, [&] { hipLaunchKernelGGL(ct::count_reduce_kernel, dim3((unsigned) ((n + 3) / 4)), dim3(256), 0, c->st, A); })) return rc;   // (four waves, four regions, per block)
	c->out.assign(n * 6, 0);
	NGM_HIP_TRY(hipMemcpyAsync(c->out.data(), c->d_out.p, n * 48, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	c->took(1, 0, 1);
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
		if (int rc = c->read_totals("ngm_count_stats", counts, 4)) return rc;
		counts[4] = c->masked_hit;
	}
	if (ms) for (int k = 0; k < 2; ++k) ms[k] = c->ms[k];
	return 0;
}
