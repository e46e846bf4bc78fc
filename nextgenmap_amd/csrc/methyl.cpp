// methyl.cpp -- host side of `ngm-hip --bs-mapping --methyl` (include/ngm_pipeline.h, ngm_methyl_*): one pair of uint32 (meth, unmeth)
// per base of the reference in HBM for the whole run, fed by every batch, and at the end of the run Bismark's cytosine report made chunk by
// chunk -- flags, select, lines -- so that the temporaries are bounded whatever the genome's size.  Kernels: csrc/methyl_device.h; the
// host-only parts (walk, context, serialiser): csrc/methyl.h; what it shares with the other side outputs: csrc/side_output.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ngm_pipeline.h"
#define NGM_METHYL_FINISH_KERNELS
#include "methyl_device.h"
#define NGM_SIDE_LINE_STREAM
#include "side_output.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace mt = ngm::met;
namespace side = ngm::side;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

struct ngm_methyl : side::Base {   // d_tot: [0] alignments [1] lines [2..7] meth, unmeth of CG, CHG, CHH; ms: [0] add [1] flags [2] select [3] text
	int min_qual = mt::kDefaultMinQual;
	uint32_t min_depth = 1, selection = mt::kSelectAll;
	std::vector<uint64_t> off;      // [n_ref + 1]
	Buf<uint32_t> cnt;              // two per base
	side::Genome genome;
	Buf<uint64_t> d_off, d_start;
	side::Names names;
	side::Staged staged;
	side::LineStream ls;            // its idx: the sites that are lines
};

namespace {
// the object over the contigs of ref; genome: a resident reference's, or null and ref's own packed words go up
ngm_methyl *create(const ngm_methyl_params *p, int device, const side::RefView &ref, const uint32_t *genome) {
	if (p->min_qual < 0 || p->min_qual > 93) { ngm::pipeline_set_error("ngm_methyl_create: min_qual is not in 0..93"); return nullptr; }
	if (p->min_depth < 0) { ngm::pipeline_set_error("ngm_methyl_create: min_depth is negative"); return nullptr; }
	const uint32_t selection = p->context ? mt::selection_of(p->context) : mt::kSelectAll;
	if (!selection) { ngm::pipeline_set_error("ngm_methyl_create: context %s is not all, CpG, CHG or CHH", p->context); return nullptr; }
	if (hipSetDevice(device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", device); return nullptr; }
	ngm_methyl *c = new ngm_methyl();
	c->n_ref = ref.n_ref();
	c->min_qual = p->min_qual; c->min_depth = (uint32_t) p->min_depth; c->selection = selection;
	c->off = mt::pair_offsets(ref.lens.data(), c->n_ref);
	const uint64_t bases = c->off[c->n_ref];
	if (c->cnt.alloc((size_t) bases * 2)) {
		ngm::pipeline_set_error("out of device memory for the methylation counters (%llu bytes: 8 per base of the reference, on device %d)", (unsigned long long) bases * 8ull, device);
		delete c;
		return nullptr;
	}
	bool ok = c->open(device, 5, 8) && c->ls.open(p->scan_chunk) && ngm::put(c->d_off, c->off, c->st) && ngm::put(c->d_start, ref.start, c->st) && c->names.upload(ref, c->st);
	ok = ok && hipMemsetAsync(c->cnt.p, 0, std::max<size_t>((size_t) bases * 8, 4), c->st) == hipSuccess;
	if (!c->ready("ngm_methyl_create", ok)) { ngm_methyl_destroy(c); return nullptr; }
	if (!c->genome.place("ngm_methyl_create", ref, genome, device)) { ngm_methyl_destroy(c); return nullptr; }
	return c;
}

mt::Layout layout_of(const ngm_methyl *c) { return mt::Layout{c->d_off.p, c->genome.p, c->d_start.p, c->n_ref, c->min_qual}; }
mt::Counters counters_of(const ngm_methyl *c) { return mt::Counters{c->cnt.p, c->d_tot.p}; }
}  // namespace

extern "C" ngm_methyl *ngm_methyl_create(const ngm_methyl_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name || !p->ref_seq))) { ngm::pipeline_set_error("ngm_methyl_create: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_arrays("ngm_methyl_create", p->n_ref, p->ref_len, p->ref_name, p->ref_seq, true, true)) return nullptr;
	return create(p, p->device, ref, nullptr);
}

extern "C" ngm_methyl *ngm_methyl_create_for_ref(const ngm_ref *r, const ngm_methyl_params *p) {
	if (!r || !p || !r->d_genome.p) { ngm::pipeline_set_error("ngm_methyl_create_for_ref: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_ref("ngm_methyl_create_for_ref", *r)) return nullptr;
	return create(p, r->device, ref, r->d_genome.p);   // (the reference outlives the run's caller)
}

extern "C" void ngm_methyl_destroy(ngm_methyl *c) { side::destroy(c); }

extern "C" int ngm_methyl_add(ngm_methyl *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
		const char *qual_text, const uint8_t *bottom, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off || !seq_off || !bottom)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_methyl_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	if (int rc = side::check_batch("ngm_methyl_add", cigar_off, cigar_text, seq_off, seq_text, qual_text, n, [&](size_t i, const char *cigar, uint32_t len, uint64_t seq_len) {   // (the checks of ngm_snp_add)
		const int why = sn::check_alignment(ref_id[i], pos0[i], cigar, len, c->n_ref, seq_len);
		return why == cv::kOk ? nullptr : sn::why(why);
	})) return rc;
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "ngm_methyl_add: add after ngm_methyl_finish")) return rc;
	DeviceGuard g(c->device);
	side::Arrays A{};
	if (int rc = c->staged.upload(c->st, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text, bottom, n, &A)) return rc;
	const mt::MethylArrays S{sn::SnpArrays{A.ref_id, A.pos0, A.cigar_off, A.cigar, A.seq_off, A.seq, A.qual, A.n}, A.reverse};
	return c->add_kernel([&] { hipLaunchKernelGGL(mt::methyl_add_kernel<mt::MethylArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, layout_of(c), counters_of(c)); });
}

// the mapper's in-place route (mapper_sam.cpp): the layout and counters its methyl_add_kernel works with
side::Base *ngm::side::base(ngm_methyl *c) { return c; }
int ngm::methyl_target(ngm_methyl *c, ngm::met::Layout *l, ngm::met::Counters *t) {
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "a batch for the methylation counters after ngm_methyl_finish")) return rc;
	*l = layout_of(c);
	*t = counters_of(c);
	return 0;
}

extern "C" int ngm_methyl_finish(ngm_methyl *c) {
	if (!c) { ngm::pipeline_set_error("ngm_methyl_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_methyl_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->staged.release();
	return c->ls.reserve_select(*c, (size_t) std::min<uint64_t>(c->ls.chunk, c->off[c->n_ref]), "out of device memory for the methylation finish (%zu bases per chunk)");
}

// the next chunk of the counters: its sites' lines into c->ls.text
static int next_chunk(ngm_methyl *c) {
	side::LineStream &ls = c->ls;
	const uint64_t s0 = ls.next_slot;
	const size_t n = (size_t) std::min<uint64_t>(ls.chunk, c->off[c->n_ref] - s0);
	mt::ChunkArgs T{};
	T.cnt = c->cnt.p; T.n = (uint32_t) n; T.s0 = s0; T.off = c->d_off.p; T.n_ref = c->n_ref; T.genome = c->genome.p; T.start = c->d_start.p;
	T.min_depth = c->min_depth; T.selection = c->selection; T.flag = ls.flag.p; T.idx = ls.idx.p; T.names = c->names.d_names.p; T.name_off = c->names.d_name_off.p;
	T.totals = c->d_tot.p + 1;
	uint32_t m = 0;
	if (int rc = ls.select_only(*c, n, [&] { hipLaunchKernelGGL(mt::methyl_flag_kernel, dim3(blocks_of(n)), dim3(256), 0, c->st, T); }, &m)) return rc;
	if (m == 0) return 0;
	return ls.lines(*c, m, "out of device memory for the lines of %u sites", [&] { T.m = m; T.len = ls.len.p; T.line_off = ls.line_off.p; hipLaunchKernelGGL(mt::methyl_lengths_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); },
			[&](char *out) { T.out = out; hipLaunchKernelGGL(mt::methyl_write_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); });
}

extern "C" long long ngm_methyl_next(ngm_methyl *c, void *out, size_t out_cap) {
	if (!c) { ngm::pipeline_set_error("ngm_methyl_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->finished) { ngm::pipeline_set_error("ngm_methyl_next: ngm_methyl_finish has not been called"); return -22; }
	DeviceGuard g(c->device);
	return c->ls.next(out, out_cap, c->off[c->n_ref], "ngm_methyl_next: ngm_methyl_finish has not succeeded", [&] { return next_chunk(c); });
}

extern "C" int ngm_methyl_stats(const ngm_methyl *c, uint64_t counts[8], float ms[4]) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);   // (ms is written under it by add, next and the mappers)
	if (counts) if (int rc = c->read_totals("ngm_methyl_stats", counts, 8)) return rc;
	if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->ms[k];
	return 0;
}
