// snp.cpp -- host side of `ngm-hip --snp` (include/ngm_pipeline.h, ngm_snp_*): coverage's difference array and three mismatch counters
// per base of the reference in HBM for the whole run, fed by every batch, and at the end of the run the VCF text made chunk by chunk --
// scan, call flags, lines -- so that the temporaries are bounded whatever the genome's size.  Kernels: csrc/snp_device.h; the host-only
// parts (walk, checks, layout, call rule, serialiser): csrc/snp.h; what it shares with the other side outputs: csrc/side_output.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ngm_pipeline.h"
#define NGM_SNP_FINISH_KERNELS
#include "snp_device.h"
#define NGM_SIDE_LINE_STREAM
#include "side_output.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace side = ngm::side;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

struct ngm_snp : side::Base {   // d_tot: [0] alignments [1] mismatching bases counted [2] calls [3] text bytes [4] covered bases
	sn::Rule rule{10u, 0.8, 15};
	std::vector<uint64_t> off;      // [n_ref + 1]
	std::string head;               // the file's header: the first piece ngm_snp_next hands out
	bool head_out = false;
	Buf<int32_t> diff;
	Buf<uint32_t> alt;
	side::Genome genome;
	Buf<uint64_t> d_off, d_start;
	side::Names names;
	side::Staged staged;
	side::LineStream ls;            // its idx: the calls
	int32_t carry = 0;              // the depth carried from chunk to chunk
};

namespace {
// the object over the contigs of ref; genome: a resident reference's, or null and ref's own packed words go up
ngm_snp *create(const ngm_snp_params *p, int device, const side::RefView &ref, const uint32_t *genome) {
	if (!(p->min_frac > 0.0 && p->min_frac <= 1.0)) { ngm::pipeline_set_error("ngm_snp_create: min_frac is not in (0, 1]"); return nullptr; }
	if (p->min_qual < 0 || p->min_qual > 93) { ngm::pipeline_set_error("ngm_snp_create: min_qual is not in 0..93"); return nullptr; }
	if (hipSetDevice(device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", device); return nullptr; }
	ngm_snp *c = new ngm_snp();
	c->n_ref = ref.n_ref();
	c->rule = sn::Rule{p->min_cov, p->min_frac, p->min_qual};
	c->off = cv::contig_offsets(ref.lens.data(), c->n_ref);
	char frac[40];
	snprintf(frac, sizeof(frac), "%g", p->min_frac);
	c->head = sn::header(c->n_ref, ref.names.data(), ref.lens.data(), c->rule, p->min_frac_text ? p->min_frac_text : frac);
	const uint64_t slots = c->off[c->n_ref];
	if (c->diff.alloc(slots) || c->alt.alloc(slots * 3)) {
		ngm::pipeline_set_error("out of device memory for the SNP counters (%llu bytes: 16 per base of the reference, on device %d)", (unsigned long long) slots * 16ull, device);
		delete c;
		return nullptr;
	}
	bool ok = c->open(device, 5, 5) && c->ls.open(p->scan_chunk) && ngm::put(c->d_off, c->off, c->st) && ngm::put(c->d_start, ref.start, c->st) && c->names.upload(ref, c->st);
	ok = ok && hipMemsetAsync(c->diff.p, 0, slots * 4, c->st) == hipSuccess && hipMemsetAsync(c->alt.p, 0, slots * 12, c->st) == hipSuccess;
	if (!c->ready("ngm_snp_create", ok)) { ngm_snp_destroy(c); return nullptr; }
	if (!c->genome.place("ngm_snp_create", ref, genome, device)) { ngm_snp_destroy(c); return nullptr; }
	return c;
}

sn::Target target_of(ngm_snp *c) { return sn::Target{c->diff.p, c->alt.p, c->d_off.p, c->genome.p, c->d_start.p, c->n_ref, c->rule.min_qual, c->d_tot.p}; }
}  // namespace

extern "C" ngm_snp *ngm_snp_create(const ngm_snp_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name || !p->ref_seq))) { ngm::pipeline_set_error("ngm_snp_create: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_arrays("ngm_snp_create", p->n_ref, p->ref_len, p->ref_name, p->ref_seq, true, true)) return nullptr;
	return create(p, p->device, ref, nullptr);
}

extern "C" ngm_snp *ngm_snp_create_for_ref(const ngm_ref *r, const ngm_snp_params *p) {
	if (!r || !p || !r->d_genome.p) { ngm::pipeline_set_error("ngm_snp_create_for_ref: bad arguments"); return nullptr; }
	side::RefView ref;
	if (!ref.from_ref("ngm_snp_create_for_ref", *r)) return nullptr;
	return create(p, r->device, ref, r->d_genome.p);   // (the reference outlives the run's caller)
}

extern "C" void ngm_snp_destroy(ngm_snp *c) { side::destroy(c); }

extern "C" int ngm_snp_add(ngm_snp *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
		const char *qual_text, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off || !seq_off)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_snp_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	if (int rc = side::check_batch("ngm_snp_add", cigar_off, cigar_text, seq_off, seq_text, qual_text, n, [&](size_t i, const char *cigar, uint32_t len, uint64_t seq_len) {
		const int why = sn::check_alignment(ref_id[i], pos0[i], cigar, len, c->n_ref, seq_len);
		return why == cv::kOk ? nullptr : sn::why(why);
	})) return rc;
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "ngm_snp_add: add after ngm_snp_finish")) return rc;
	DeviceGuard g(c->device);
	side::Arrays A{};
	if (int rc = c->staged.upload(c->st, ref_id, pos0, cigar_off, cigar_text, seq_off, seq_text, qual_text, nullptr, n, &A)) return rc;
	const sn::SnpArrays S{A.ref_id, A.pos0, A.cigar_off, A.cigar, A.seq_off, A.seq, A.qual, A.n};
	return c->add_kernel([&] { hipLaunchKernelGGL(sn::snp_add_kernel<sn::SnpArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, target_of(c)); });
}

// the mapper's in-place route (mapper_sam.cpp): where its snp_add_kernel adds
side::Base *ngm::side::base(ngm_snp *c) { return c; }
int ngm::snp_target(ngm_snp *c, ngm::snp::Target *t) {
	std::unique_lock<std::mutex> lk;
	if (int rc = c->begin_add(lk, "a batch for the SNP counters after ngm_snp_finish")) return rc;
	*t = target_of(c);
	return 0;
}

extern "C" int ngm_snp_finish(ngm_snp *c) {
	if (!c) { ngm::pipeline_set_error("ngm_snp_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_snp_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->staged.release();
	return c->ls.reserve(*c, (size_t) std::min<uint64_t>(c->ls.chunk, c->off[c->n_ref]), "out of device memory for the SNP scan (%zu slots per chunk)");
}

// the next chunk of the arrays: its calls' lines into c->ls.text
static int scan_chunk(ngm_snp *c) {
	side::LineStream &ls = c->ls;
	const uint64_t s0 = ls.next_slot;
	const size_t n = (size_t) std::min<uint64_t>(ls.chunk, c->off[c->n_ref] - s0);
	sn::ChunkArgs T{};
	T.depth = c->diff.p + s0; T.alt = c->alt.p + 3u * s0; T.n = (uint32_t) n; T.s0 = s0; T.off = c->d_off.p; T.n_ref = c->n_ref; T.genome = c->genome.p; T.start = c->d_start.p;
	T.rule = c->rule; T.flag = ls.flag.p; T.idx = ls.idx.p; T.names = c->names.d_names.p; T.name_off = c->names.d_name_off.p; T.totals = c->d_tot.p + 2;
	uint32_t m = 0;
	if (int rc = ls.scan_and_select(*c, c->diff.p + s0, c->carry, n, [&] { hipLaunchKernelGGL(sn::snp_flag_kernel, dim3(blocks_of(n)), dim3(256), 0, c->st, T); }, &m, &c->carry)) return rc;
	if (m == 0) return 0;
	return ls.lines(*c, m, "out of device memory for the lines of %u calls", [&] { T.m = m; T.len = ls.len.p; T.line_off = ls.line_off.p; hipLaunchKernelGGL(sn::snp_lengths_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); },
			[&](char *out) { T.out = out; hipLaunchKernelGGL(sn::snp_write_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T); });
}

extern "C" long long ngm_snp_next(ngm_snp *c, void *out, size_t out_cap) {
	if (!c) { ngm::pipeline_set_error("ngm_snp_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->finished) { ngm::pipeline_set_error("ngm_snp_next: ngm_snp_finish has not been called"); return -22; }
	DeviceGuard g(c->device);
	if (!c->head_out) {   // the header is the first piece
		c->ls.text.assign(c->head.begin(), c->head.end());
		c->ls.text_at = 0;
		c->head_out = true;
	}
	return c->ls.next(out, out_cap, c->off[c->n_ref], "ngm_snp_next: ngm_snp_finish has not succeeded", [&] { return scan_chunk(c); });
}

extern "C" int ngm_snp_stats(const ngm_snp *c, uint64_t counts[5], float ms[4]) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);   // (ms and head_out are written under it by add, next and the mappers)
	if (counts) {
		if (int rc = c->read_totals("ngm_snp_stats", counts, 5)) return rc;
		if (c->head_out) counts[3] += c->head.size();   // (the header is made on the host)
	}
	if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->ms[k];
	return 0;
}
