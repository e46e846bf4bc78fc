// mapper_sam.cpp -- the write_sam stage of a map call (map_impl, mapper.cpp): the batch's records as SAM / BAM text on the GPU
// (sam_device.h), the side outputs --coverage / --snp / --count / --methyl from the same arrays, and where the text goes: the caller's buffer,
// the BGZF compressor or the sorter.  With it the SAM entry points that need no map call: ngm_mapper_set_sam_options, ngm_mapper_sam_fetch.
#define NGM_SAM_KERNELS
#include "mapper_internal.h"
#define NGM_COV_BATCH_KERNELS
#include "coverage_device.h"
#include "snp_device.h"
#include "count_device.h"
#include "methyl_device.h"
#include "side_output.h"
#include <rocprim/rocprim.hpp>

namespace ngm {
namespace {

// The side outputs (--coverage, --snp, --count, --methyl) of a SAM batch whose object lives on another device than the mapper: cov_mask_kernel has
// said which records count; they, the CIGAR texts and, for --snp, --count and --methyl, the read rows come down and go through ngm_*_add.
int side_outputs_away(ngm_mapper *m, bool cov_away, bool snp_away, bool count_away, bool methyl_away, int n, int q, int units, bool paired, const ngm_hit *hits, const ngm::SamRef *sam_refs,
		size_t str_bytes, const SamCall *sam) {
	// the object lives on another device: which reads count and the CIGAR texts come down
	m->cov_mask.resize((size_t) units); m->cov_text.resize(str_bytes + 1);
	MAP_HIP_TRY(hipMemcpy(m->cov_mask.data(), m->d_cov_mask.p, (size_t) units, hipMemcpyDeviceToHost));
	if (str_bytes) MAP_HIP_TRY(hipMemcpy(m->cov_text.data(), m->d_str.p, str_bytes, hipMemcpyDeviceToHost));
	if (cov_away) {
		// ... and the arrays go through ngm_coverage_add
		m->cov_ref.clear(); m->cov_pos.clear(); m->cov_off.clear();
		std::vector<char> packed;
		const int per = paired ? 2 : 1;
		for (int u = 0; u < units; ++u) for (int k = 0; k < per; ++k) {
			if (!((m->cov_mask[u] >> k) & 1)) continue;
			const int i = per * u + k;
			m->cov_ref.push_back(hits[i].contig); m->cov_pos.push_back((int32_t) hits[i].pos); m->cov_off.push_back((uint32_t) packed.size());
			packed.insert(packed.end(), m->cov_text.data() + sam_refs[i].cig_off, m->cov_text.data() + sam_refs[i].cig_off + sam_refs[i].cig_len);
		}
		m->cov_off.push_back((uint32_t) packed.size());
		if (int rc = ngm_coverage_add(m->coverage, m->cov_ref.data(), m->cov_pos.data(), m->cov_off.data(), packed.data(), m->cov_ref.size())) return rc;
	}
	if (snp_away || count_away || methyl_away) {
		// ... with the read rows; the sequences and qualities are put as the records print them (bam_mapped, sam_device.h) and the arrays
		// go through ngm_snp_add, ngm_count_add (with the records' strands) and ngm_methyl_add (top or bottom: the strand, the other way
		// round for a pair's second mate) -- the records with a quality string and those without one in
		// a call each
		m->snp_rows.resize((size_t) n * q);
		MAP_HIP_TRY(hipMemcpy(m->snp_rows.data(), m->batch_reads, (size_t) n * q, hipMemcpyDeviceToHost));
		const ngm::SamMeta *meta = (const ngm::SamMeta *) sam->meta;
		const uint8_t *quals = (const uint8_t *) sam->quals;
		const int per = paired ? 2 : 1;
		const bool clip = m->prm.hard_clip || m->prm.silent_clip;
		for (int with_q = 0; with_q < 2; ++with_q) {
			std::vector<int32_t> s_ref, s_pos;
			std::vector<uint32_t> c_off, s_off;
			std::vector<uint8_t> s_rev, s_bot;
			std::string c_text, s_text, q_text;
			for (int u = 0; u < units; ++u) for (int k = 0; k < per; ++k) {
				if (!((m->cov_mask[u] >> k) & 1)) continue;
				const int i = per * u + k;
				const int qlen = meta[i].qual_len & 0x7FFF;
				if ((qlen != 0) != (with_q != 0)) continue;
				const uint8_t *row = m->snp_rows.data() + (size_t) i * q, *qrow = quals + (size_t) i * q;
				const int L = (int) strnlen((const char *) row, (size_t) q);
				const int s0 = std::max(0, std::min(clip ? hits[i].qstart : 0, L));
				const int sl = std::max(0, std::min(clip ? L - hits[i].qstart - hits[i].qend : L, L - s0));
				const int QL = std::min(qlen, L);
				s_ref.push_back(hits[i].contig); s_pos.push_back((int32_t) hits[i].pos); c_off.push_back((uint32_t) c_text.size()); s_off.push_back((uint32_t) s_text.size());
				s_rev.push_back(hits[i].reverse ? 1 : 0);
				s_bot.push_back(((hits[i].reverse != 0) != (paired && k == 1)) ? 1 : 0);
				c_text.append(m->cov_text.data() + sam_refs[i].cig_off, sam_refs[i].cig_len);
				for (int t = 0; t < sl; ++t) {
					if (!hits[i].reverse) { s_text.push_back((char) row[s0 + t]); if (with_q) q_text.push_back(s0 + t < QL ? (char) qrow[s0 + t] : ':'); }
					else {
						const char ch = (char) row[L - 1 - (s0 + t)];
						s_text.push_back(ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch);
						if (with_q) q_text.push_back(QL - 1 - (s0 + t) >= 0 ? (char) qrow[QL - 1 - (s0 + t)] : ':');
					}
				}
			}
			c_off.push_back((uint32_t) c_text.size()); s_off.push_back((uint32_t) s_text.size());
			if (s_ref.empty()) continue;
			if (snp_away) if (int rc = ngm_snp_add(m->snp, s_ref.data(), s_pos.data(), c_off.data(), c_text.data(), s_off.data(), s_text.data(), with_q ? q_text.c_str() : nullptr, s_ref.size())) return rc;
			if (count_away) if (int rc = ngm_count_add(m->count, s_ref.data(), s_pos.data(), c_off.data(), c_text.data(), s_off.data(), s_text.data(), with_q ? q_text.c_str() : nullptr, s_rev.data(), s_ref.size())) return rc;
			if (methyl_away) if (int rc = ngm_methyl_add(m->methyl, s_ref.data(), s_pos.data(), c_off.data(), c_text.data(), s_off.data(), s_text.data(), with_q ? q_text.c_str() : nullptr, s_bot.data(), s_ref.size())) return rc;
		}
	}
	return 0;
}

// the byte stream grows by the host-built strings (rare: strings beyond the device's scratch rows)
int append_host_strings(MapBatch &b) {
	ngm_mapper *m = b.m;
	const uint64_t str_base = b.str_base;
	const std::vector<char> &extra = b.extra;
	const size_t need = (size_t) str_base + extra.size();
	if (need > m->d_str.cap) {
		ngm::DevBuf<char> bigger;
		MAP_OOM_TRY(bigger.reserve(need + 4096), "out of device memory (SAM strings)");
		if (str_base) MAP_HIP_TRY(hipMemcpyAsync(bigger.p, m->d_str.p, (size_t) str_base, hipMemcpyDeviceToDevice, m->st));
		MAP_HIP_TRY(hipStreamSynchronize(m->st));
		std::swap(bigger, m->d_str);   // (the smaller one goes with `bigger`, here)
	}
	MAP_OOM_TRY(m->p_sam_extra.reserve(extra.size()), "out of pinned host memory");
	memcpy(m->p_sam_extra.p, extra.data(), extra.size());
	MAP_HIP_TRY(hipMemcpyAsync(m->d_str.p + str_base, m->p_sam_extra.p, extra.size(), hipMemcpyHostToDevice, m->st));
	return 0;
}

ngm::SamArgs sam_args(const MapBatch &b) {
	ngm_mapper *m = b.m;
	const ngm_ref *r = m->ref;
	const int n = b.n, q = b.q;
	const bool paired = b.paired;
	const SamCall *sam = b.sam;
	ngm::SamArgs S{};
	S.n = n; S.q = q; S.paired = paired ? 1 : 0;
	S.unit_len_bound = (uint32_t) ((paired ? 2 : 1) * (2 * q + 1024));
	S.reads = m->batch_reads; S.quals = m->d_sam_quals.p; S.names = m->d_sam_names.p; S.meta = m->d_sam_meta.p; S.hits = m->d_sam_hits.p; S.refs = m->d_sam_refs.p;
	S.str = m->d_str.p; S.contig_names = m->d_sam_contig_names.p; S.contig_name_off = m->d_sam_contig_off.p;
	S.min_insert = m->sam_opt.min_insert_size; S.max_insert = m->sam_opt.max_insert_size > 0 ? m->sam_opt.max_insert_size : 2147483647;
	S.min_mq = m->sam_opt.min_mq; S.no_unal = m->sam_opt.no_unal; S.hard_clip = m->prm.hard_clip; S.silent_clip = m->prm.silent_clip;
	S.min_identity = m->sam_opt.min_identity; S.min_residues = m->sam_opt.min_residues;
	S.rg = m->sam_rg.empty() ? nullptr : m->d_sam_rg.p; S.rg_len = (int) m->sam_rg.size(); S.bs_mapping = m->sam_opt.bs_mapping;
	S.slam_seq = m->sam_opt.slam_seq; S.variant_cpu = m->prm.variant == NGM_VARIANT_OCL_CPU ? 1 : 0; S.alt_scoring = (m->prm.bs_mapping || (m->prm.slam_seq & 2)) ? 1 : 0;
	S.genome = r->d_genome.p; S.contig_start = m->d_sam_contig_start.p;
	S.unit_len = m->d_sam_len.p; S.unit_off = m->d_sam_off.p; S.counters = m->d_total.p + 16;
	S.bam = m->sam_opt.bam ? 1 : 0;
	S.polya = sam->polya ? m->d_sam_polya.p : nullptr;
	return S;
}

// The text kernels' launch sequence, shared by write_sam and the test hook ngm_debug_sam_records: lengths per unit, exclusive prefix sum, the
// 32-bit total checked against the 64-bit sum, bytes.  S is complete but for `out` (unit_len / unit_off are sc.len / sc.off, reserved for
// units + 1 elements; counters zeroed); *total: bytes of text in sc.text.  stage: the turn taken again in front of the write kernel, or null.
struct SamScratch { ngm::DevBuf<uint32_t> &len, &off; ngm::DevBuf<uint8_t> &scan_tmp; ngm::DevBuf<char> &text; };
int sam_text_kernels(ngm::SamArgs &S, int units, const SamScratch &sc, hipStream_t st, GpuStage *stage, const char *who, unsigned long long *total) {
	const bool bam_slam = S.bam && S.slam_seq;   // (BAM records with SLAM-seq tags: kernels of their own, sam_device.h)
	if (bam_slam) hipLaunchKernelGGL(ngm::sam_lengths_kernel<true>, dim3((units + 255) / 256), dim3(256), 0, st, S, units);
	else hipLaunchKernelGGL(ngm::sam_lengths_kernel<false>, dim3((units + 255) / 256), dim3(256), 0, st, S, units);
	MAP_HIP_TRY(hipGetLastError());
	size_t tmp_bytes = 0;
	(void) rocprim::exclusive_scan(nullptr, tmp_bytes, sc.len.p, sc.off.p, 0u, (size_t) units + 1, rocprim::plus<uint32_t>(), st);
	MAP_OOM_TRY(sc.scan_tmp.reserve(tmp_bytes + 16), "out of device memory (scan)");
	MAP_HIP_TRY(hipMemsetAsync(sc.len.p + units, 0, 4, st));
	MAP_HIP_TRY(rocprim::exclusive_scan(sc.scan_tmp.p, tmp_bytes, sc.len.p, sc.off.p, 0u, (size_t) units + 1, rocprim::plus<uint32_t>(), st));
	uint32_t total32 = 0;
	unsigned long long total64 = 0;
	MAP_HIP_TRY(hipMemcpyAsync(&total32, sc.off.p + units, 4, hipMemcpyDeviceToHost, st));
	MAP_HIP_TRY(hipMemcpyAsync(&total64, S.counters + 3, 8, hipMemcpyDeviceToHost, st));
	MAP_HIP_TRY(hipStreamSynchronize(st));
	if (total64 != (unsigned long long) total32) {   // the 32-bit prefix sums have wrapped (detected directly, not through a per-record bound)
		ngm::pipeline_set_error("%s: the text of this batch of %d reads is %llu bytes, beyond the 32-bit offsets of a batch: use smaller batches", who, S.n, total64);
		return -75;
	}
	*total = total32;
	MAP_OOM_TRY(sc.text.reserve((size_t) *total + 16), "out of device memory (SAM text)");
	S.out = sc.text.p;
	if (stage) stage->acquire();
	if (bam_slam) hipLaunchKernelGGL(ngm::sam_write_kernel<true>, dim3((units + 255) / 256), dim3(256), 0, st, S, units);
	else hipLaunchKernelGGL(ngm::sam_write_kernel<false>, dim3((units + 255) / 256), dim3(256), 0, st, S, units);
	MAP_HIP_TRY(hipGetLastError());
	return 0;
}

// --coverage, --snp, --count, --methyl: the records just written as mapped ones add to the run's counters on this device
// (coverage_device.h: their blocks; snp_device.h: their depth blocks and their mismatching, qualifying columns; count_device.h: their
// eligible columns and their regions' read counts; methyl_device.h: their calls over the reference's C or G), from the same arrays, before the batch's buffers are reused (behind e1: not part of the SAM stage's time)
struct SideAdds {
	ngm_mapper *m; const ngm::SamArgs &S; const int units;
	ngm::side::Base *const cov_b = ngm::side::base(m->coverage), *const snp_b = ngm::side::base(m->snp), *const count_b = ngm::side::base(m->count),
			*const methyl_b = ngm::side::base(m->methyl);
	bool here(const ngm::side::Base *b) const { return b && units > 0 && ngm::side::device(b) == m->ref->device; }
	const bool cov_away = cov_b && units > 0 && !here(cov_b), snp_away = snp_b && units > 0 && !here(snp_b), count_away = count_b && units > 0 && !here(count_b),
			methyl_away = methyl_b && units > 0 && !here(methyl_b);
	template <typename L> int add_here(ngm::side::Base *b, hipEvent_t *ev, L launch) {   // (nothing for an object that is elsewhere)
		if (!here(b)) return 0;
		MAP_HIP_TRY(hipEventRecord(ev[0], m->st));
		launch();
		MAP_HIP_TRY(hipGetLastError());
		MAP_HIP_TRY(hipEventRecord(ev[1], m->st));
		return 0;
	}
	void note_here(ngm::side::Base *b, hipEvent_t *ev) { float t = 0; if (here(b) && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) ngm::side::note_add_ms(b, t); }
	int enqueue() {
		ngm::cov::Target cov_to{};
		if (here(cov_b)) if (int rc = ngm::coverage_target(m->coverage, &cov_to)) return rc;
		if (int rc = add_here(cov_b, m->cev + 2, [&] {
			hipLaunchKernelGGL(ngm::cov::cov_add_kernel<ngm::cov::CovBatch>, dim3((units + 255) / 256), dim3(256), 0, m->st, ngm::cov::CovBatch{S, units, cov_to.off}, cov_to.counters, cov_to.off, cov_to.n_ref, cov_to.n_aln);
		})) return rc;
		ngm::snp::Target snp_to{};
		if (here(snp_b)) if (int rc = ngm::snp_target(m->snp, &snp_to)) return rc;
		if (int rc = add_here(snp_b, m->cev + 4, [&] {
			hipLaunchKernelGGL(ngm::snp::snp_add_kernel<ngm::snp::SnpBatch>, dim3((units + 255) / 256), dim3(256), 0, m->st, ngm::snp::SnpBatch{S, units}, snp_to);
		})) return rc;
		ngm::cnt::Layout count_tab{};
		ngm::cnt::Counters count_to{};
		if (here(count_b)) if (int rc = ngm::count_target(m->count, &count_tab, &count_to)) return rc;
		if (int rc = add_here(count_b, m->cev + 6, [&] {
			hipLaunchKernelGGL(ngm::cnt::count_add_kernel<ngm::cnt::CountBatch>, dim3((units + 255) / 256), dim3(256), 0, m->st, ngm::cnt::CountBatch{ngm::snp::SnpBatch{S, units}}, count_tab, count_to);
		})) return rc;
		ngm::met::Layout methyl_tab{};
		ngm::met::Counters methyl_to{};
		if (here(methyl_b)) if (int rc = ngm::methyl_target(m->methyl, &methyl_tab, &methyl_to)) return rc;
		if (int rc = add_here(methyl_b, m->cev + 8, [&] {
			hipLaunchKernelGGL(ngm::met::methyl_add_kernel<ngm::met::MethylBatch>, dim3((units + 255) / 256), dim3(256), 0, m->st, ngm::met::MethylBatch{ngm::snp::SnpBatch{S, units}}, methyl_tab, methyl_to);
		})) return rc;
		if (cov_away || snp_away || count_away || methyl_away) {
			MAP_OOM_TRY(m->d_cov_mask.reserve((size_t) units), "out of device memory (coverage)");
			hipLaunchKernelGGL(ngm::cov::cov_mask_kernel, dim3((units + 255) / 256), dim3(256), 0, m->st, S, units, m->d_cov_mask.p);
			MAP_HIP_TRY(hipGetLastError());
		}
		return 0;
	}
	void note() { note_here(cov_b, m->cev + 2); note_here(snp_b, m->cev + 4); note_here(count_b, m->cev + 6); note_here(methyl_b, m->cev + 8); }
};

// the records stay in HBM: their BGZF blocks are written there too (bgzf_device.h, the compressor's own stream -- beside the next
// instance's kernels), and only those travel
int route_bam(MapBatch &b, unsigned long long total, int units, float *bgzf_ms) {
	ngm_mapper *m = b.m;
	const ngm_ref *r = m->ref;
	SamCall *sam = b.sam;
	if (m->sorter) {
		// --sort: the records stay in HBM for the whole run (bam_sort.cpp); nothing travels now
		int rc;
		if (ngm::bam_sort_device(m->sorter) == r->device) rc = ngm::bam_sort_add_device(m->sorter, m->batch_seq, m->d_sam_text.p, (size_t) total, m->d_sam_off.p, (size_t) units);
		else {
			m->sorter_host.resize((size_t) total);
			MAP_HIP_TRY(hipMemcpy(m->sorter_host.data(), m->d_sam_text.p, (size_t) total, hipMemcpyDeviceToHost));
			rc = ngm_bam_sort_add(m->sorter, m->batch_seq, m->sorter_host.data(), (size_t) total);
		}
		if (rc < 0) return rc == -12 ? -28 : rc;   // (-28: the sorter is full -- not one of the mapper's own allocations, which say -12)
		sam->text_bytes = 0;
		m->sam_text_bytes = 0;
	} else if (sam->out_cap < ngm_bgzf_bound((size_t) total)) sam->text_bytes = (long long) ngm_bgzf_bound((size_t) total);   // (> out_cap: ngm_mapper_sam_fetch with a buffer of that size)
	else {
		const long long zlen = ngm_bgzf_compress_device(m->bz, m->d_sam_text.p, (size_t) total, sam->out, sam->out_cap);
		if (zlen < 0) return (int) zlen;
		sam->text_bytes = zlen;
		m->sam_text_bytes = 0;
		*bgzf_ms = ngm_bgzf_last_kernel_ms(m->bz);
	}
	return 0;
}

}  // namespace

// ---- SAM text on the GPU: lengths per unit, exclusive prefix sum, bytes (sam_device.h) ------------------------------
int write_sam(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n, q = b.q;
	const bool paired = b.paired;
	SamCall *sam = b.sam;
	ngm_hit *hits = b.hits;
	ngm::SamRef *sam_refs = b.sam_refs;
	GpuStage stage_sam(m, 1, false, 2);
	const int units = paired ? n / 2 : n;
	if (!b.extra.empty()) if (int rc = append_host_strings(b)) return rc;
	MAP_OOM_TRY(m->d_sam_len.reserve((size_t) units + 1) || m->d_sam_off.reserve((size_t) units + 1), "out of device memory (SAM stage)");
	MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_hits.p, hits, (size_t) n * sizeof(ngm_hit), hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_refs.p, sam_refs, (size_t) n * sizeof(ngm::SamRef), hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemsetAsync(m->d_total.p + 16, 0, 64, m->st));
	MAP_HIP_TRY(hipStreamSynchronize(m->st));   // (the uploads -- 64 bytes per read -- travel outside the stage lock)
	stage_sam.acquire();
	ngm::SamArgs S = sam_args(b);
	hipEvent_t e0 = m->cev[0], e1 = m->cev[1];
	MAP_HIP_TRY(hipEventRecord(e0, m->st));
	unsigned long long total = 0;
	if (units > 0) if (int rc = sam_text_kernels(S, units, SamScratch{m->d_sam_len, m->d_sam_off, m->d_scan_tmp, m->d_sam_text}, m->st, &stage_sam, "ngm_mapper_map_sam", &total)) return rc;
	MAP_HIP_TRY(hipEventRecord(e1, m->st));
	SideAdds side{m, S, units};
	if (int rc = side.enqueue()) return rc;
	unsigned long long ctr[7] = {0, 0, 0, 0, 0, 0, 0};
	MAP_HIP_TRY(hipMemcpyAsync(ctr, m->d_total.p + 16, 56, hipMemcpyDeviceToHost, m->st));
	m->sam_text_bytes = total;
	const bool bam = m->sam_opt.bam != 0;
	if (!bam && total <= sam->out_cap && total > 0) MAP_HIP_TRY(hipMemcpyAsync(sam->out, m->d_sam_text.p, (size_t) total, hipMemcpyDeviceToHost, m->st));
	stage_sam.done_after(e1);   // the text (~420 bytes per read) travels while the next instance's kernels run
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	sam->text_bytes = (long long) total;
	side.note();
	if (side.cov_away || side.snp_away || side.count_away || side.methyl_away)
		if (int rc = side_outputs_away(m, side.cov_away, side.snp_away, side.count_away, side.methyl_away, n, q, units, paired, hits, sam_refs, (size_t) b.str_base + b.extra.size(), sam)) return rc;
	float bgzf_ms = 0.f;
	if (bam && total > 0) if (int rc = route_bam(b, total, units, &bgzf_ms)) return rc;
	if (sam->stats) { sam->stats[0] = ctr[0]; sam->stats[1] = ctr[1]; sam->stats[2] = ctr[2]; }
	m->pair_stats[0] = ctr[4]; m->pair_stats[1] = ctr[5]; m->pair_stats[2] = ctr[6];
	float t = 0;
	sam->kernel_ms = (hipEventElapsedTime(&t, e0, e1) == hipSuccess ? t : 0.f) + bgzf_ms;
	b.lap(5);
	return 0;
}

}  // namespace ngm

extern "C" {

int ngm_mapper_set_sam_options(ngm_mapper *m, const ngm_sam_options *o) {
	if (!m || !o) return -22;
	ngm::DevGuard g(m->ref->device);
	m->sam_opt = *o;
	m->sam_opt.rg_id = nullptr;
	if (o->bam && !m->bz) { m->bz = ngm_bgzf_create(m->ref->device); if (!m->bz) return -12; }
	m->sam_rg = o->rg_id ? o->rg_id : "";
	const ngm_ref *r = m->ref;
	std::string names;
	std::vector<uint32_t> off(r->contigs.size() + 1, 0);
	for (size_t i = 0; i < r->contigs.size(); ++i) { off[i] = (uint32_t) names.size(); names += r->contigs[i].name; }
	off[r->contigs.size()] = (uint32_t) names.size();
	MAP_OOM_TRY(m->d_sam_contig_names.reserve(names.size() + 16) || m->d_sam_contig_off.reserve(off.size()) || m->d_sam_rg.reserve(m->sam_rg.size() + 16), "out of device memory (SAM options)");
	MAP_HIP_TRY(hipMemcpy(m->d_sam_contig_names.p, names.data(), names.size(), hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(m->d_sam_contig_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
	if (!m->sam_rg.empty()) MAP_HIP_TRY(hipMemcpy(m->d_sam_rg.p, m->sam_rg.data(), m->sam_rg.size(), hipMemcpyHostToDevice));
	{
		std::vector<uint64_t> starts(r->contigs.size() + 1, 0);
		for (size_t i = 0; i < r->contigs.size(); ++i) starts[i] = r->contigs[i].start;
		MAP_OOM_TRY(m->d_sam_contig_start.reserve(starts.size()), "out of device memory (SAM options)");
		MAP_HIP_TRY(hipMemcpy(m->d_sam_contig_start.p, starts.data(), starts.size() * 8, hipMemcpyHostToDevice));
	}
	m->sam_ready = true;
	return 0;
}

int ngm_mapper_sam_fetch(ngm_mapper *m, char *out, size_t out_cap) {
	if (!m || !out || out_cap < m->sam_text_bytes) return -22;
	ngm::DevGuard g(m->ref->device);
	if (m->sam_opt.bam && !m->argos_text) {   // the last call's records are still in HBM: their BGZF blocks into the larger buffer; returns their length
		if (!m->sam_text_bytes) return 0;
		const long long zlen = ngm_bgzf_compress_device(m->bz, m->d_sam_text.p, (size_t) m->sam_text_bytes, out, out_cap);
		if (zlen < 0 || zlen > 0x7fffffffll) return zlen < 0 ? (int) zlen : -75;
		m->sam_text_bytes = 0;
		return (int) zlen;
	}
	if (m->sam_text_bytes) MAP_HIP_TRY(hipMemcpy(out, m->d_sam_text.p, (size_t) m->sam_text_bytes, hipMemcpyDeviceToHost));
	return 0;
}

// test hook: the record writers over constructed hits.  Everything the kernels index with is checked here first; then the uploads and
// sam_text_kernels, the launch sequence of write_sam.
long long ngm_debug_sam_records(int device, const ngm_sam_options *opt, int hard_clip, int silent_clip, int variant, int alt_scoring, int n, int q,
		const char *reads, const char *quals, const char *names, size_t names_bytes, const ngm_sam_read *meta, const ngm_hit *hits, const char *const *cigars,
		const char *const *mds, const uint16_t *polya, int n_contigs, const char *const *contig_names, const uint64_t *contig_lens, const ngm_ref *ref,
		char *out, size_t out_cap, unsigned long long counters[7]) {
	const char *fn = "ngm_debug_sam_records";
	if (!opt || n < 0 || q < 1 || q > 0x7FFF || n_contigs < 0 || !counters || (out_cap && !out) || (n && (!reads || !quals || !meta || !hits || !cigars || !mds)) || (names_bytes && !names) ||
			(n_contigs && (!contig_names || !contig_lens)) || (opt->paired && (n & 1))) { ngm::pipeline_set_error("%s: bad arguments", fn); return -22; }
	const std::string rg = opt->rg_id ? opt->rg_id : "";
	std::string cnames, str;
	std::vector<uint32_t> cname_off((size_t) n_contigs + 1, 0);
	std::vector<uint64_t> cstart((size_t) n_contigs + 1, 0);
	for (int c = 0; c < n_contigs; ++c) {
		if (!contig_names[c]) { ngm::pipeline_set_error("%s: contig %d has no name", fn, c); return -22; }
		cname_off[c] = (uint32_t) cnames.size(); cnames += contig_names[c];
	}
	cname_off[n_contigs] = (uint32_t) cnames.size();
	if (opt->slam_seq) {   // the tags read the packed genome: the reference's contigs are the table's
		if (!ref || ref->device != device || !ref->d_genome.p || (int) ref->contigs.size() != n_contigs) { ngm::pipeline_set_error("%s: slam_seq needs a reference on device %d whose contigs are the table's", fn, device); return -22; }
		for (int c = 0; c < n_contigs; ++c) {
			const NgmContig &rc = ref->contigs[c];
			if (rc.name != contig_names[c] || rc.len != contig_lens[c] || rc.start + rc.len > ref->genome_words * 8ull) { ngm::pipeline_set_error("%s: contig %d differs from the reference's", fn, c); return -22; }
			cstart[c] = rc.start;
		}
	}
	std::vector<ngm::SamRef> refs((size_t) n);
	for (int i = 0; i < n; ++i) {
		const ngm_sam_read &mt = meta[i];
		const ngm_hit &h = hits[i];
		if ((uint64_t) mt.name_off + mt.name_len > names_bytes) { ngm::pipeline_set_error("%s: read %d: its name ends beyond names_bytes", fn, i); return -22; }
		if (mt.name_len > 254) { ngm::pipeline_set_error("%s: read %d: a name of %d bytes (BAM's l_read_name is one byte)", fn, i, (int) mt.name_len); return -22; }
		const char *cg = cigars[i] ? cigars[i] : "", *md = mds[i] ? mds[i] : "";
		const size_t cl = strlen(cg), ml = strlen(md);
		if (cl > 0xFFFF || ml > 0xFFFF || str.size() + cl + ml > 0xFFFFFFFFull) { ngm::pipeline_set_error("%s: read %d: CIGAR or MD too long", fn, i); return -22; }
		refs[i] = ngm::SamRef{(uint32_t) str.size(), (uint32_t) (str.size() + cl), (uint16_t) cl, (uint16_t) ml};
		str.append(cg, cl); str.append(md, ml);
		if (!h.mapped) continue;   // (no writer looks at the rest of a hit without `mapped`)
		const int L = (int) strnlen(reads + (size_t) i * q, (size_t) q);
		if (h.contig < 0 || h.contig >= n_contigs) { ngm::pipeline_set_error("%s: read %d: contig %d is not in the table", fn, i, h.contig); return -22; }
		if (h.qstart < 0 || h.qend < 0 || (long long) h.qstart + h.qend > L) { ngm::pipeline_set_error("%s: read %d: clipped %d + %d of %d bases", fn, i, h.qstart, h.qend, L); return -22; }
		unsigned long long num = 0, read_used = 0, span = 0;
		bool digits = false;
		for (size_t c = 0; c < cl; ++c) {
			const char ch = cg[c];
			if (ch >= '0' && ch <= '9') { num = num * 10ull + (unsigned long long) (ch - '0'); digits = true; if (num >= (1ull << 28)) break; continue; }
			if (!digits || !strchr("MIDNSHP=X", ch)) { num = 1ull << 28; break; }
			if (ch == 'M' || ch == 'I') read_used += num;
			if (ch == 'M' || ch == 'D' || ch == 'N' || ch == '=' || ch == 'X') span += num;
			num = 0; digits = false;
		}
		if (num >= (1ull << 28) || digits) { ngm::pipeline_set_error("%s: read %d: malformed CIGAR", fn, i); return -22; }
		if (read_used > (unsigned long long) (L - h.qstart)) { ngm::pipeline_set_error("%s: read %d: its CIGAR consumes %llu bases, %d follow the clipped start", fn, i, read_used, L - h.qstart); return -22; }
		if (opt->slam_seq && (h.pos > contig_lens[h.contig] || span > contig_lens[h.contig] - h.pos)) { ngm::pipeline_set_error("%s: read %d: the alignment ends beyond its contig", fn, i); return -22; }
	}
	const int units = opt->paired ? n / 2 : n;
	const size_t rows = std::max<size_t>((size_t) n * (size_t) q, 1), nn = std::max<size_t>((size_t) n, 1);
	ngm::DevGuard g(device);
	ngm::DevBuf<uint8_t> d_reads, d_quals, d_scan_tmp;
	ngm::DevBuf<char> d_names, d_str, d_cnames, d_rg, d_text;
	ngm::DevBuf<ngm::SamMeta> d_meta;
	ngm::DevBuf<ngm_hit> d_hits;
	ngm::DevBuf<ngm::SamRef> d_refs;
	ngm::DevBuf<uint32_t> d_coff, d_len, d_off;
	ngm::DevBuf<uint64_t> d_cstart;
	ngm::DevBuf<uint16_t> d_polya;
	ngm::DevBuf<unsigned long long> d_ctr;
	unsigned long long total = 0;
	if (d_reads.reserve(rows) || d_quals.reserve(rows) || d_names.reserve(names_bytes + 16) || d_str.reserve(str.size() + 16) || d_cnames.reserve(cnames.size() + 16) || d_rg.reserve(rg.size() + 16) ||
			d_meta.reserve(nn) || d_hits.reserve(nn) || d_refs.reserve(nn) || d_coff.reserve(cname_off.size()) || d_cstart.reserve(cstart.size()) || d_polya.reserve(nn) ||
			d_len.reserve((size_t) units + 1) || d_off.reserve((size_t) units + 1) || d_ctr.reserve(8)) { ngm::pipeline_set_error("out of device memory (%s)", fn); return -12; }
	if (n) {
		MAP_HIP_TRY(hipMemcpy(d_reads.p, reads, (size_t) n * q, hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_quals.p, quals, (size_t) n * q, hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_meta.p, meta, (size_t) n * sizeof(ngm::SamMeta), hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_hits.p, hits, (size_t) n * sizeof(ngm_hit), hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_refs.p, refs.data(), (size_t) n * sizeof(ngm::SamRef), hipMemcpyHostToDevice));
		if (polya) MAP_HIP_TRY(hipMemcpy(d_polya.p, polya, (size_t) n * 2, hipMemcpyHostToDevice));
	}
	if (names_bytes) MAP_HIP_TRY(hipMemcpy(d_names.p, names, names_bytes, hipMemcpyHostToDevice));
	if (!str.empty()) MAP_HIP_TRY(hipMemcpy(d_str.p, str.data(), str.size(), hipMemcpyHostToDevice));
	if (!cnames.empty()) MAP_HIP_TRY(hipMemcpy(d_cnames.p, cnames.data(), cnames.size(), hipMemcpyHostToDevice));
	if (!rg.empty()) MAP_HIP_TRY(hipMemcpy(d_rg.p, rg.data(), rg.size(), hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_coff.p, cname_off.data(), cname_off.size() * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_cstart.p, cstart.data(), cstart.size() * 8, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemset(d_ctr.p, 0, 64));
	MAP_HIP_TRY(hipDeviceSynchronize());
	ngm::SamArgs S{};   // as sam_args fills it from a mapper
	S.n = n; S.q = q; S.paired = opt->paired ? 1 : 0;
	S.unit_len_bound = (uint32_t) ((opt->paired ? 2 : 1) * (2 * q + 1024));
	S.reads = d_reads.p; S.quals = d_quals.p; S.names = d_names.p; S.meta = d_meta.p; S.hits = d_hits.p; S.refs = d_refs.p;
	S.str = d_str.p; S.contig_names = d_cnames.p; S.contig_name_off = d_coff.p;
	S.min_insert = opt->min_insert_size; S.max_insert = opt->max_insert_size > 0 ? opt->max_insert_size : 2147483647;
	S.min_mq = opt->min_mq; S.no_unal = opt->no_unal; S.hard_clip = hard_clip; S.silent_clip = silent_clip;
	S.min_identity = opt->min_identity; S.min_residues = opt->min_residues;
	S.rg = rg.empty() ? nullptr : d_rg.p; S.rg_len = (int) rg.size(); S.bs_mapping = opt->bs_mapping;
	S.slam_seq = opt->slam_seq; S.variant_cpu = variant == NGM_VARIANT_OCL_CPU ? 1 : 0; S.alt_scoring = alt_scoring ? 1 : 0;
	S.genome = opt->slam_seq ? ref->d_genome.p : nullptr; S.contig_start = d_cstart.p;
	S.unit_len = d_len.p; S.unit_off = d_off.p; S.counters = d_ctr.p;
	S.bam = opt->bam ? 1 : 0;
	S.polya = polya ? d_polya.p : nullptr;
	if (units > 0) if (int rc = ngm::sam_text_kernels(S, units, ngm::SamScratch{d_len, d_off, d_scan_tmp, d_text}, 0, nullptr, fn, &total)) return rc;
	MAP_HIP_TRY(hipDeviceSynchronize());
	MAP_HIP_TRY(hipMemcpy(counters, d_ctr.p, 56, hipMemcpyDeviceToHost));
	if (total && total <= out_cap) MAP_HIP_TRY(hipMemcpy(out, d_text.p, (size_t) total, hipMemcpyDeviceToHost));
	return (long long) total;
}

}  // extern "C"
