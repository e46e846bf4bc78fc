// snp.cpp -- host side of `ngm-hip --snp` (include/ngm_pipeline.h, ngm_snp_*): coverage's difference array and three mismatch counters
// per base of the reference in HBM for the whole run, fed by every batch, and at the end of the run the VCF text made chunk by chunk --
// scan, call flags, lines -- so that the temporaries are bounded whatever the genome's size.  Kernels: csrc/snp_device.h; the host-only
// parts (walk, checks, layout, call rule, serialiser): csrc/snp.h.
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
#define NGM_SNP_FINISH_KERNELS
#include "snp_device.h"
#include "device_util.h"
#include "refindex.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

namespace {
constexpr size_t kDefaultChunk = (size_t) 1 << 25;   // slots scanned at a time
constexpr size_t kMaxChunk = (size_t) 1 << 30;       // (the calls' chunk offsets are 32-bit)
}  // namespace

struct ngm_snp {
	int device = 0, n_ref = 0;
	size_t chunk = kDefaultChunk;
	sn::Rule rule{10u, 0.8, 15};
	std::vector<uint64_t> off;      // [n_ref + 1]
	std::string head;               // the file's header: the first piece ngm_snp_next hands out
	std::mutex mu;
	hipStream_t st = nullptr;
	hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	Buf<int32_t> diff;
	Buf<uint32_t> alt;
	Buf<uint32_t> own_genome;       // the packed reference, unless a resident one is used
	const uint32_t *genome = nullptr;
	Buf<uint64_t> d_off, d_start;
	Buf<char> d_names;
	Buf<uint32_t> d_name_off;
	Buf<unsigned long long> d_tot;  // [0] alignments [1] mismatching bases counted [2] calls [3] text bytes [4] covered bases
	bool finished = false, head_out = false;
	// scratch of add (under mu)
	Buf<int32_t> a_ref, a_pos;
	Buf<uint32_t> a_off, a_soff;
	Buf<char> a_text, a_seq, a_qual;
	// the finish: temporaries of a chunk, the depth carried from chunk to chunk, the chunk's text on the host
	Buf<uint8_t> flag, tmp;
	Buf<uint32_t> idx, len, d_m;
	Buf<uint64_t> line_off;
	Buf<char> d_text;
	uint64_t next_slot = 0;
	int32_t carry = 0;
	std::vector<char> text;
	size_t text_at = 0;
	float ms[4] = {0, 0, 0, 0};
};

namespace {
// everything but the packed reference: the contigs' table, the counters, the header
ngm_snp *create_common(const ngm_snp_params *p, int device, int n_ref, const uint32_t *ref_len, const char *const *ref_name, const std::vector<uint64_t> &start) {
	if (!(p->min_frac > 0.0 && p->min_frac <= 1.0)) { ngm::pipeline_set_error("ngm_snp_create: min_frac is not in (0, 1]"); return nullptr; }
	if (p->min_qual < 0 || p->min_qual > 93) { ngm::pipeline_set_error("ngm_snp_create: min_qual is not in 0..93"); return nullptr; }
	if (hipSetDevice(device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", device); return nullptr; }
	ngm_snp *c = new ngm_snp();
	c->device = device;
	c->n_ref = n_ref;
	c->chunk = std::min(p->scan_chunk ? p->scan_chunk : kDefaultChunk, kMaxChunk);
	c->rule = sn::Rule{p->min_cov, p->min_frac, p->min_qual};
	c->off = cv::contig_offsets(ref_len, n_ref);
	char frac[40];
	snprintf(frac, sizeof(frac), "%g", p->min_frac);
	c->head = sn::header(n_ref, ref_name, ref_len, c->rule, p->min_frac_text ? p->min_frac_text : frac);
	const uint64_t slots = c->off[n_ref];
	std::string names;
	std::vector<uint32_t> name_off((size_t) n_ref + 1, 0);
	for (int k = 0; k < n_ref; ++k) { names += ref_name[k]; name_off[(size_t) k + 1] = (uint32_t) names.size(); }
	if (c->diff.alloc(slots) || c->alt.alloc(slots * 3)) {
		ngm::pipeline_set_error("out of device memory for the SNP counters (%llu bytes: 16 per base of the reference, on device %d)", (unsigned long long) slots * 16ull, device);
		delete c;
		return nullptr;
	}
	bool ok = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) == hipSuccess;
	for (hipEvent_t &e : c->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	ok = ok && !c->d_off.alloc(c->off.size()) && !c->d_start.alloc(start.size()) && !c->d_names.alloc(names.size()) && !c->d_name_off.alloc(name_off.size()) && !c->d_tot.alloc(5) && !c->d_m.alloc(1);
	ok = ok && hipMemsetAsync(c->diff.p, 0, slots * 4, c->st) == hipSuccess && hipMemsetAsync(c->alt.p, 0, slots * 12, c->st) == hipSuccess && hipMemsetAsync(c->d_tot.p, 0, 40, c->st) == hipSuccess;
	ok = ok && hipMemcpyAsync(c->d_off.p, c->off.data(), c->off.size() * 8, hipMemcpyHostToDevice, c->st) == hipSuccess;
	ok = ok && hipMemcpyAsync(c->d_start.p, start.data(), start.size() * 8, hipMemcpyHostToDevice, c->st) == hipSuccess;
	ok = ok && (names.empty() || hipMemcpyAsync(c->d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->st) == hipSuccess);
	ok = ok && hipMemcpyAsync(c->d_name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, c->st) == hipSuccess;
	ok = ok && hipStreamSynchronize(c->st) == hipSuccess;   // (the host arrays are free again; the counters are zero before a mapper's stream adds to them)
	if (!ok) { ngm::pipeline_set_error("ngm_snp_create: set-up failed on device %d (%s)", device, hipGetErrorString(hipGetLastError())); ngm_snp_destroy(c); return nullptr; }
	return c;
}
}  // namespace

extern "C" ngm_snp *ngm_snp_create(const ngm_snp_params *p) {
	if (!p || p->n_ref < 0 || (p->n_ref > 0 && (!p->ref_len || !p->ref_name || !p->ref_seq))) { ngm::pipeline_set_error("ngm_snp_create: bad arguments"); return nullptr; }
	for (int c = 0; c < p->n_ref; ++c) {
		if (!p->ref_name[c]) { ngm::pipeline_set_error("ngm_snp_create: contig %d has no name", c); return nullptr; }
		if (!p->ref_seq[c] || strnlen(p->ref_seq[c], (size_t) p->ref_len[c]) != (size_t) p->ref_len[c]) { ngm::pipeline_set_error("ngm_snp_create: the sequence of contig %d is shorter than its length", c); return nullptr; }
	}
	std::vector<uint64_t> start;
	const std::vector<uint32_t> words = sn::pack_reference(p->ref_seq, p->ref_len, p->n_ref, start);
	ngm_snp *c = create_common(p, p->device, p->n_ref, p->ref_len, p->ref_name, start);
	if (!c) return nullptr;
	if (c->own_genome.alloc(words.size()) || hipMemcpy(c->own_genome.p, words.data(), words.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
		ngm::pipeline_set_error("ngm_snp_create: the packed reference (%zu bytes) could not be placed on device %d", words.size() * 4, p->device);
		ngm_snp_destroy(c);
		return nullptr;
	}
	c->genome = c->own_genome.p;
	return c;
}

extern "C" ngm_snp *ngm_snp_create_for_ref(const ngm_ref *r, const ngm_snp_params *p) {
	if (!r || !p || !r->d_genome) { ngm::pipeline_set_error("ngm_snp_create_for_ref: bad arguments"); return nullptr; }
	const int n_ref = (int) r->contigs.size();
	std::vector<uint32_t> lens((size_t) n_ref);
	std::vector<const char *> names((size_t) n_ref);
	std::vector<uint64_t> start((size_t) n_ref + 1, 0);
	for (int c = 0; c < n_ref; ++c) {
		if (r->contigs[c].len > 0xffffffffull || r->contigs[c].start + r->contigs[c].len > r->genome_words * 8ull) { ngm::pipeline_set_error("ngm_snp_create_for_ref: contig %d does not fit", c); return nullptr; }
		lens[c] = (uint32_t) r->contigs[c].len; names[c] = r->contigs[c].name.c_str(); start[c] = r->contigs[c].start;
	}
	start[n_ref] = r->genome_words * 8ull;
	ngm_snp *c = create_common(p, r->device, n_ref, lens.data(), names.data(), start);
	if (c) c->genome = r->d_genome;   // (the reference outlives the run's caller)
	return c;
}

extern "C" void ngm_snp_destroy(ngm_snp *c) {
	if (!c) return;
	DeviceGuard g(c->device);
	if (c->st) (void) hipStreamSynchronize(c->st);
	for (hipEvent_t e : c->ev) if (e) (void) hipEventDestroy(e);
	if (c->st) (void) hipStreamDestroy(c->st);
	delete c;   // (the buffers free themselves: the device is still this one)
}

namespace {
sn::Target target_of(ngm_snp *c) { return sn::Target{c->diff.p, c->alt.p, c->d_off.p, c->genome, c->d_start.p, c->n_ref, c->rule.min_qual, c->d_tot.p}; }
}  // namespace

extern "C" int ngm_snp_add(ngm_snp *c, const int32_t *ref_id, const int32_t *pos0, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text,
		const char *qual_text, size_t n) {
	if (!c || (n && (!ref_id || !pos0 || !cigar_off || !seq_off)) || n > 0x7fffffffu) { ngm::pipeline_set_error("ngm_snp_add: bad arguments"); return -22; }
	if (n == 0) return 0;
	// the checks need no lock: they are over the caller's memory, before anything of it reaches the device
	const size_t qual_len = qual_text ? strlen(qual_text) : 0;
	for (size_t i = 0; i < n; ++i) {
		if (cigar_off[i + 1] < cigar_off[i] || (cigar_off[i + 1] > cigar_off[i] && !cigar_text)) { ngm::pipeline_set_error("ngm_snp_add: alignment %zu: its CIGAR offsets do not ascend", i); return -22; }
		if (seq_off[i + 1] < seq_off[i] || (seq_off[i + 1] > seq_off[i] && !seq_text)) { ngm::pipeline_set_error("ngm_snp_add: alignment %zu: its sequence offsets do not ascend", i); return -22; }
		const int why = sn::check_alignment(ref_id[i], pos0[i], cigar_text + cigar_off[i], cigar_off[i + 1] - cigar_off[i], c->n_ref, (uint64_t) (seq_off[i + 1] - seq_off[i]));
		if (why != cv::kOk) { ngm::pipeline_set_error("ngm_snp_add: alignment %zu: %s", i, sn::why(why)); return -22; }
		// (a quality text is a C string under the sequence's offsets: the first alignment it does not reach is the one refused)
		if (qual_text && (size_t) seq_off[i + 1] > qual_len) { ngm::pipeline_set_error("ngm_snp_add: alignment %zu: %s", i, sn::why(sn::kQualLength)); return -22; }
	}
	if (qual_text && qual_len != (size_t) seq_off[n]) { ngm::pipeline_set_error("ngm_snp_add: alignment %zu: %s", n - 1, sn::why(sn::kQualLength)); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_snp_add: add after ngm_snp_finish"); return -22; }
	DeviceGuard g(c->device);
	const size_t t0 = cigar_off[0], tn = cigar_off[n] - t0, s0 = seq_off[0], sn_bytes = seq_off[n] - s0;
	if (c->a_ref.grow(n) || c->a_pos.grow(n) || c->a_off.grow(n + 1) || c->a_soff.grow(n + 1) || c->a_text.grow(tn + 1) || c->a_seq.grow(sn_bytes + 1) || (qual_text && c->a_qual.grow(sn_bytes + 1))) {
		ngm::pipeline_set_error("out of device memory for %zu alignments", n);
		return -12;
	}
	NGM_HIP_TRY(hipMemcpyAsync(c->a_ref.p, ref_id, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_pos.p, pos0, n * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_off.p, cigar_off, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
	NGM_HIP_TRY(hipMemcpyAsync(c->a_soff.p, seq_off, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
	if (tn) NGM_HIP_TRY(hipMemcpyAsync(c->a_text.p, cigar_text + t0, tn, hipMemcpyHostToDevice, c->st));
	if (sn_bytes) NGM_HIP_TRY(hipMemcpyAsync(c->a_seq.p, seq_text + s0, sn_bytes, hipMemcpyHostToDevice, c->st));
	if (sn_bytes && qual_text) NGM_HIP_TRY(hipMemcpyAsync(c->a_qual.p, qual_text + s0, sn_bytes, hipMemcpyHostToDevice, c->st));
	// (the offsets count from the caller's first byte)
	sn::SnpArrays S{c->a_ref.p, c->a_pos.p, c->a_off.p, c->a_text.p - t0, c->a_soff.p, c->a_seq.p - s0, qual_text ? c->a_qual.p - s0 : nullptr, (uint32_t) n};
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	hipLaunchKernelGGL(sn::snp_add_kernel<sn::SnpArrays>, dim3(blocks_of(n)), dim3(256), 0, c->st, S, target_of(c));
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	float t = 0.f;
	if (hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[0] += t;
	return 0;
}

// the mapper's in-place route (mapper.cpp): where its snp_add_kernel adds, and the time that kernel took
int ngm::snp_device(const ngm_snp *c) { return c ? c->device : -1; }
int ngm::snp_target(ngm_snp *c, ngm::snp::Target *t) {
	if (!c) return -22;
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("a batch for the SNP counters after ngm_snp_finish"); return -22; }
	*t = target_of(c);
	return 0;
}
void ngm::snp_note_add_ms(ngm_snp *c, float ms) {
	if (!c) return;
	std::lock_guard<std::mutex> lk(c->mu);
	c->ms[0] += ms;
}

extern "C" int ngm_snp_finish(ngm_snp *c) {
	if (!c) { ngm::pipeline_set_error("ngm_snp_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->finished) { ngm::pipeline_set_error("ngm_snp_finish: called twice"); return -22; }
	c->finished = true;
	DeviceGuard g(c->device);
	NGM_HIP_TRY(hipDeviceSynchronize());   // (the mappers' streams on this device have added their last batch)
	c->a_ref.release(); c->a_pos.release(); c->a_off.release(); c->a_soff.release(); c->a_text.release(); c->a_seq.release(); c->a_qual.release();
	const size_t n = (size_t) std::min<uint64_t>(c->chunk, c->off[c->n_ref]);
	size_t tb = 0, tb2 = 0;
	NGM_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, (int32_t *) nullptr, (int32_t *) nullptr, (int32_t) 0, n, rocprim::plus<int32_t>(), c->st));
	NGM_HIP_TRY(rocprim::select(nullptr, tb2, rocprim::counting_iterator<uint32_t>(0), (uint8_t *) nullptr, (uint32_t *) nullptr, (uint32_t *) nullptr, n, c->st));
	if (c->flag.alloc(n) || c->idx.alloc(n) || c->tmp.alloc(std::max(tb, tb2) + 16)) { ngm::pipeline_set_error("out of device memory for the SNP scan (%zu slots per chunk)", n); return -12; }
	return 0;
}

namespace {
// the next chunk of the arrays: its calls' lines into c->text
int scan_chunk(ngm_snp *c) {
	const uint64_t s0 = c->next_slot;
	const size_t n = (size_t) std::min<uint64_t>(c->chunk, c->off[c->n_ref] - s0);
	int32_t *depth = c->diff.p + s0;
	size_t tb = c->tmp.n;
	NGM_HIP_TRY(hipEventRecord(c->ev[0], c->st));
	NGM_HIP_TRY(rocprim::inclusive_scan(c->tmp.p, tb, depth, depth, c->carry, n, rocprim::plus<int32_t>(), c->st));   // (in place, the depth in front carried in)
	NGM_HIP_TRY(hipEventRecord(c->ev[1], c->st));
	sn::ChunkArgs T{};
	T.depth = depth; T.alt = c->alt.p + 3u * s0; T.n = (uint32_t) n; T.s0 = s0; T.off = c->d_off.p; T.n_ref = c->n_ref; T.genome = c->genome; T.start = c->d_start.p;
	T.rule = c->rule; T.flag = c->flag.p; T.idx = c->idx.p; T.names = c->d_names.p; T.name_off = c->d_name_off.p; T.totals = c->d_tot.p + 2;
	hipLaunchKernelGGL(sn::snp_flag_kernel, dim3(blocks_of(n)), dim3(256), 0, c->st, T);
	NGM_HIP_TRY(hipGetLastError());
	tb = c->tmp.n;
	NGM_HIP_TRY(rocprim::select(c->tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), c->flag.p, c->idx.p, c->d_m.p, n, c->st));
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
	c->carry = last_depth;
	if (m == 0) return 0;
	if (c->len.grow((size_t) m + 1) || c->line_off.grow((size_t) m + 1)) { ngm::pipeline_set_error("out of device memory for the lines of %u calls", m); return -12; }
	T.m = m; T.len = c->len.p; T.line_off = c->line_off.p;
	NGM_HIP_TRY(hipEventRecord(c->ev[3], c->st));
	NGM_HIP_TRY(hipMemsetAsync(c->len.p + m, 0, 4, c->st));
	hipLaunchKernelGGL(sn::snp_lengths_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T);
	NGM_HIP_TRY(hipGetLastError());
	auto widen = rocprim::make_transform_iterator(c->len.p, [] __host__ __device__ (uint32_t x) { return (uint64_t) x; });
	size_t sb = 0;
	NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, sb, widen, c->line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), c->st));
	if (c->tmp.grow(sb + 16)) { ngm::pipeline_set_error("out of device memory for a scan"); return -12; }
	NGM_HIP_TRY(rocprim::exclusive_scan(c->tmp.p, sb, widen, c->line_off.p, (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), c->st));
	uint64_t total = 0;
	NGM_HIP_TRY(hipMemcpyAsync(&total, c->line_off.p + m, 8, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	if (total) {
		if (c->d_text.grow((size_t) total)) { ngm::pipeline_set_error("out of device memory for %llu bytes of lines", (unsigned long long) total); return -12; }
		T.out = c->d_text.p;
		hipLaunchKernelGGL(sn::snp_write_kernel, dim3(blocks_of(m)), dim3(256), 0, c->st, T);
		NGM_HIP_TRY(hipGetLastError());
	}
	NGM_HIP_TRY(hipEventRecord(c->ev[4], c->st));
	c->text.resize((size_t) total);
	if (total) NGM_HIP_TRY(hipMemcpyAsync(c->text.data(), c->d_text.p, (size_t) total, hipMemcpyDeviceToHost, c->st));
	NGM_HIP_TRY(hipStreamSynchronize(c->st));
	if (hipEventElapsedTime(&t, c->ev[3], c->ev[4]) == hipSuccess) c->ms[3] += t;
	return 0;
}
}  // namespace

extern "C" long long ngm_snp_next(ngm_snp *c, void *out, size_t out_cap) {
	if (!c) { ngm::pipeline_set_error("ngm_snp_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(c->mu);
	if (!c->finished) { ngm::pipeline_set_error("ngm_snp_next: ngm_snp_finish has not been called"); return -22; }
	DeviceGuard g(c->device);
	if (!c->head_out) {   // the header is the first piece
		c->text.assign(c->head.begin(), c->head.end());
		c->text_at = 0;
		c->head_out = true;
	}
	while (c->text_at >= c->text.size()) {
		if (c->next_slot >= c->off[c->n_ref]) return 0;
		if (!c->flag.p) { ngm::pipeline_set_error("ngm_snp_next: ngm_snp_finish has not succeeded"); return -22; }
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

extern "C" int ngm_snp_stats(const ngm_snp *c, uint64_t counts[5], float ms[4]) {
	if (!c) return -22;
	if (counts) {
		DeviceGuard g(c->device);
		unsigned long long h[5] = {0, 0, 0, 0, 0};
		if (hipMemcpy(h, c->d_tot.p, 40, hipMemcpyDeviceToHost) != hipSuccess) { ngm::pipeline_set_error("ngm_snp_stats: the counters could not be read (%s)", hipGetErrorString(hipGetLastError())); return -5; }
		for (int k = 0; k < 5; ++k) counts[k] = h[k];
		if (c->head_out) counts[3] += c->head.size();   // (the header is made on the host)
	}
	if (ms) for (int k = 0; k < 4; ++k) ms[k] = c->ms[k];
	return 0;
}
