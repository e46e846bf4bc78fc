// mapper_argos.cpp -- `--argos` (include/ngm_pipeline.h: ngm_mapper_set_argos, ngm_mapper_map_argos, ngm_argos_prolog,
// ngm_mapper_argos_counters): the candidate search and BatchScore of the SAM path, then every candidate of a read ordered by score and
// printed as ScoreWriter's line on the GPU (argos_device.h).  No selection, no alignment: the reference's ScoreBuffer hands the sorted
// read straight to the writer (src/ScoreBuffer.cpp:150-183, src/AlignmentBuffer.cpp:43-46).
#include "mapper_internal.h"
#include <rocprim/rocprim.hpp>
#include "argos_device.h"

using ngm::DevGuard;
using ngm::GpuStage;

namespace {
inline uint64_t pow2_at_least(uint32_t v) { uint64_t p = 1; while (p < v) p <<= 1; return p; }

// ScoreBuffer.cpp:171/179: std::sort(sortLocationScore) over the survivors v (candidate indices) in the reference's candidate order --
// libstdc++'s introsort, unstable above 16 elements: the same algorithm on the same sequence moves the elements the same way.  A list
// with an unknown rank keeps the position order (index order); returns false then.
bool argos_sort_like_reference(std::vector<uint32_t> &v, const float *score, const uint32_t *rank) {
	struct Rec { float s; uint32_t i; };
	thread_local std::vector<Rec> recs;
	bool known = rank != nullptr;
	for (uint32_t c : v) known = known && rank[c] != ngm::kArgosRankUnknown;
	if (known) std::sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return rank[x] < rank[y]; });
	else std::sort(v.begin(), v.end());
	recs.resize(v.size());
	for (size_t x = 0; x < v.size(); ++x) recs[x] = Rec{score[v[x]], v[x]};
	std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.s > b.s; });   // sortLocationScore
	for (size_t x = 0; x < v.size(); ++x) v[x] = recs[x].i;
	return known;
}

// the reads of `list` whose lists exceed the LDS cap: their scratch slices (a power of two of keys each) and one workgroup each
int argos_long_launch(ngm_mapper *m, ngm::ArgosArgs A, const std::vector<uint32_t> &list) {
	if (list.empty()) return 0;
	std::vector<uint64_t> off(list.size());
	uint64_t total = 0;
	for (size_t j = 0; j < list.size(); ++j) { off[j] = total; total += pow2_at_least(m->h_count[list[j]]); }
	if (m->d_argos_llist.reserve(list.size()) || m->d_argos_loff.reserve(list.size()) || m->d_argos_gkeys.reserve(total) || m->d_argos_gvals.reserve(total)) {
		ngm::pipeline_set_error("out of device memory (argos long lists)"); return -12; }
	MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_llist.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_loff.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, m->st));
	A.long_list = m->d_argos_llist.p; A.long_off = m->d_argos_loff.p; A.g_keys = m->d_argos_gkeys.p; A.g_vals = m->d_argos_gvals.p;
	hipLaunchKernelGGL(ngm::argos_order_kernel<true>, dim3((unsigned) list.size()), dim3(ngm::kArgosThreadsGlobal), 0, m->st, A);
	MAP_HIP_TRY(hipGetLastError());
	MAP_HIP_TRY(hipStreamSynchronize(m->st));   // (list / off are the caller's host memory)
	m->argos_long += list.size();
	return 0;
}
}  // namespace

extern "C" {

int ngm_mapper_set_argos(ngm_mapper *m, float min_score) {
	if (!m) return -22;
	if (min_score < 0.f) { m->argos_on = false; return 0; }
	if (m->prm.bs_mapping || m->prm.slam_seq) { ngm::pipeline_set_error("ngm_mapper_set_argos: --argos with --bs-mapping / --slam-seq is not supported"); return -22; }
	DevGuard g(m->ref->device);
	const std::vector<uint64_t> &st = m->ref->start_pos;
	if (st.empty() || m->d_argos_starts.reserve(st.size())) { ngm::pipeline_set_error("out of device memory (argos)"); return -12; }
	MAP_HIP_TRY(hipMemcpy(m->d_argos_starts.p, st.data(), st.size() * 8, hipMemcpyHostToDevice));
	for (auto &e : m->aev) if (!e) MAP_HIP_TRY(hipEventCreate(&e));
	m->argos_n_starts = (int) st.size();
	m->argos_min = min_score;
	m->argos_on = true;
	return 0;
}

long long ngm_mapper_map_argos(ngm_mapper *m, int n, const char *reads, const char *names, size_t names_bytes, const ngm_sam_read *meta,
		char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms) {
	if (!m || n < 0 || (n > 0 && (!reads || !meta || (names_bytes && !names)))) return -22;
	if (!m->argos_on) { ngm::pipeline_set_error("ngm_mapper_map_argos: call ngm_mapper_set_argos first"); return -22; }
	if (stats) stats[0] = stats[1] = stats[2] = 0;
	if (kernel_ms) *kernel_ms = 0.f;
	m->argos_text = true;
	m->sam_text_bytes = 0;
	if (n == 0) return 0;
	DevGuard g(m->ref->device);
	for (auto &x : m->ms) x = 0.f;
	m->order_ms = 0.f;
	const int q = m->prm.qry_max_len;
	if (m->d_reads.reserve((size_t) n * q) || m->d_sam_names.reserve(names_bytes + 16) || m->d_sam_meta.reserve(n) || m->d_argos_nsurv.reserve(n) ||
			m->d_argos_npos.reserve(n) || m->d_argos_cls.reserve(n) || m->p_argos_cls.reserve(n) || m->p_argos_nsurv.reserve(n) ||
			m->d_sam_len.reserve((size_t) n + 1) || m->d_sam_off.reserve((size_t) n + 1) || m->d_argos_ctr.reserve(4)) {
		ngm::pipeline_set_error("out of memory (argos)"); return -12; }
	m->batch_reads = m->d_reads.p;
	MAP_HIP_TRY(hipEventRecord(m->ev[0], m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->d_reads.p, reads, (size_t) n * q, hipMemcpyHostToDevice, m->st));
	if (names_bytes) MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_names.p, names, names_bytes, hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_meta.p, meta, (size_t) n * sizeof(ngm_sam_read), hipMemcpyHostToDevice, m->st));
	GpuStage stage(m);
	m->cs_paired = false;
	if (int rc = ngm::run_cs(m, n, &stage)) return rc;
	MAP_HIP_TRY(hipEventRecord(m->ev[1], m->st));
	const uint64_t np = m->n_cand;
	if (np >= 0xFFFFFFFFull) { ngm::pipeline_set_error("ngm_mapper_map_argos: %llu candidates in one batch: use smaller batches", (unsigned long long) np); return -75; }
	if (m->d_argos_ord.reserve(np + 1)) { ngm::pipeline_set_error("out of device memory (argos)"); return -12; }
	stage.acquire();
	if (np > 0) {
		if (m->d_pair_read.reserve(np) || m->d_scores.reserve(np)) { ngm::pipeline_set_error("out of device memory (score stage)"); return -12; }
		if (int rc = ngm::engine_reserve(m->eng, (int) np)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(m->eng)); return rc; }
		if (int rc = ngm::score_candidates(m, n, np, 0)) return rc;
	}

	// ---- order, pass 1: filter, sort by (score desc, candidate index), classify --------------------------------------------------------
	const uint32_t cap = (uint32_t) std::max<long>(1, std::min<long>(ngm::kArgosLdsCap, ngm::test_limit("argos_lds_cap", ngm::kArgosLdsCap)));
	const uint32_t lds_keys = (uint32_t) pow2_at_least(cap);
	ngm::ArgosArgs A{};
	A.n = n; A.list = nullptr; A.cand_base = m->d_cand_base.p; A.cand_count = m->d_cand_count.p; A.scores = m->d_scores.p; A.read_len = m->d_read_len.p;
	A.rank = nullptr; A.min_opt = m->argos_min; A.match = (float) m->prm.match_bonus; A.lds_cap = cap; A.lds_keys = lds_keys;
	A.ord = m->d_argos_ord.p; A.n_surv = m->d_argos_nsurv.p; A.n_pos = m->d_argos_npos.p; A.cls = m->d_argos_cls.p; A.counters = m->d_argos_ctr.p;
	MAP_HIP_TRY(hipMemsetAsync(m->d_argos_ctr.p, 0, 4 * sizeof(unsigned long long), m->st));
	MAP_HIP_TRY(hipEventRecord(m->aev[0], m->st));
	hipLaunchKernelGGL(ngm::argos_order_kernel<false>, dim3((unsigned) n), dim3(ngm::kArgosThreadsLds), (size_t) lds_keys * 12, m->st, A);
	MAP_HIP_TRY(hipGetLastError());
	std::vector<uint32_t> longs;
	for (int i = 0; i < n; ++i) if (m->h_count[i] > cap) longs.push_back((uint32_t) i);
	if (int rc = argos_long_launch(m, A, longs)) return rc;
	MAP_HIP_TRY(hipEventRecord(m->aev[1], m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->p_argos_cls.p, m->d_argos_cls.p, (size_t) n, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(m->p_argos_nsurv.p, m->d_argos_nsurv.p, (size_t) n * 4, hipMemcpyDeviceToHost, m->st));
	stage.done_after(m->aev[1]);
	MAP_HIP_TRY(hipStreamSynchronize(m->st));

	// ---- the reads whose order needs the reference's candidate list: S on the device (LDS, or the long-list path), H on the host -------------
	uint64_t cls_n[3] = {0, 0, 0};
	std::vector<uint32_t> need, s_lds, s_long, h_list;
	for (int i = 0; i < n; ++i) {
		if (m->p_argos_nsurv.p[i] == 0) continue;
		const uint8_t c = m->p_argos_cls.p[i];
		++cls_n[c];
		if (c == ngm::kArgosU) continue;
		need.push_back((uint32_t) i);
		if (c == ngm::kArgosH) h_list.push_back((uint32_t) i);
		else if (m->h_count[i] > cap) s_long.push_back((uint32_t) i);
		else s_lds.push_back((uint32_t) i);
	}
	GpuStage stage_txt(m, 1, false, 2);
	if (!need.empty()) {
		uint32_t *h_rank = nullptr;
		if (int rc = ngm::candidate_order(m, need, np, &h_rank)) return rc;
		stage_txt.acquire();
		ngm::ArgosArgs R = A;
		R.rank = m->d_cand_rank.p;
		if (!s_lds.empty()) {
			if (m->d_argos_list.reserve(s_lds.size())) { ngm::pipeline_set_error("out of device memory (argos)"); return -12; }
			MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_list.p, s_lds.data(), s_lds.size() * 4, hipMemcpyHostToDevice, m->st));
			R.list = m->d_argos_list.p; R.n = (int) s_lds.size();
			hipLaunchKernelGGL(ngm::argos_order_kernel<false>, dim3((unsigned) s_lds.size()), dim3(ngm::kArgosThreadsLds), (size_t) lds_keys * 12, m->st, R);
			MAP_HIP_TRY(hipGetLastError());
		}
		if (int rc = argos_long_launch(m, R, s_long)) return rc;
		if (!h_list.empty()) {
			// the survivors are entries [0, n_surv) of ord (pass 1); a read with an unknown rank keeps the position order (counted)
			if (m->p_scores.reserve(np + 1) || m->p_rec.reserve(np + 1)) { ngm::pipeline_set_error("out of pinned host memory"); return -12; }
			MAP_HIP_TRY(hipMemcpyAsync(m->p_scores.p, m->d_scores.p, np * 4, hipMemcpyDeviceToHost, m->st));
			MAP_HIP_TRY(hipMemcpyAsync(m->p_rec.p, m->d_argos_ord.p, np * 4, hipMemcpyDeviceToHost, m->st));
			MAP_HIP_TRY(hipStreamSynchronize(m->st));
			const float *hs = m->p_scores.p;
			const uint32_t *hord = reinterpret_cast<const uint32_t *>(m->p_rec.p);
			std::vector<uint32_t> hoff(h_list.size() + 1, 0);
			for (size_t j = 0; j < h_list.size(); ++j) hoff[j + 1] = hoff[j] + m->p_argos_nsurv.p[h_list[j]];
			std::vector<uint32_t> sorted(hoff.back());
			std::atomic<uint64_t> unknown{0};
			ngm::ThreadPool::instance().parallel_for((int) h_list.size(), [&](int lo, int hi) {
				std::vector<uint32_t> v;
				for (int j = lo; j < hi; ++j) {
					const uint32_t b = m->h_base[h_list[j]], ns = hoff[j + 1] - hoff[j];
					v.assign(hord + b, hord + b + ns);
					if (!argos_sort_like_reference(v, hs, h_rank)) ++unknown;
					std::copy(v.begin(), v.end(), sorted.begin() + hoff[j]);
				}
			}, 64);
			m->argos_unknown += unknown.load();
			if (m->d_argos_list.reserve(h_list.size()) || m->d_argos_hoff.reserve(hoff.size()) || m->d_argos_hord.reserve(sorted.size() + 1)) {
				ngm::pipeline_set_error("out of device memory (argos)"); return -12; }
			MAP_HIP_TRY(hipStreamSynchronize(m->st));   // (the S launch above may still read d_argos_list)
			MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_list.p, h_list.data(), h_list.size() * 4, hipMemcpyHostToDevice, m->st));
			MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_hoff.p, hoff.data(), hoff.size() * 4, hipMemcpyHostToDevice, m->st));
			if (!sorted.empty()) MAP_HIP_TRY(hipMemcpyAsync(m->d_argos_hord.p, sorted.data(), sorted.size() * 4, hipMemcpyHostToDevice, m->st));
			hipLaunchKernelGGL(ngm::argos_scatter_kernel, dim3((unsigned) h_list.size()), dim3(64), 0, m->st, (int) h_list.size(), (const uint32_t *) m->d_argos_list.p,
					(const uint32_t *) m->d_argos_hoff.p, (const uint32_t *) m->d_argos_hord.p, (const uint32_t *) m->d_cand_base.p, m->d_argos_ord.p);
			MAP_HIP_TRY(hipGetLastError());
			MAP_HIP_TRY(hipStreamSynchronize(m->st));   // (h_list, hoff, sorted are host memory of this scope)
		}
	}

	// ---- the text: lengths, exclusive scan, write (as sam_lengths_kernel / sam_write_kernel) ---------------------------------------------
	stage_txt.acquire();
	ngm::ArgosText T{};
	T.n = n; T.cand_base = m->d_cand_base.p; T.n_surv = m->d_argos_nsurv.p; T.n_pos = m->d_argos_npos.p; T.ord = m->d_argos_ord.p;
	T.loc = m->d_out_loc.p; T.sv = m->d_out_sv.p; T.scores = m->d_scores.p; T.names = m->d_sam_names.p;
	T.meta = reinterpret_cast<const uint32_t *>(m->d_sam_meta.p); T.starts = m->d_argos_starts.p; T.n_starts = m->argos_n_starts;
	T.len = m->d_sam_len.p; T.off = m->d_sam_off.p; T.counters = m->d_argos_ctr.p + 1;
	MAP_HIP_TRY(hipEventRecord(m->aev[2], m->st));
	hipLaunchKernelGGL(ngm::argos_lengths_kernel, dim3((n + 255) / 256), dim3(256), 0, m->st, T);
	MAP_HIP_TRY(hipGetLastError());
	MAP_HIP_TRY(hipMemsetAsync(m->d_sam_len.p + n, 0, 4, m->st));
	size_t tmp_bytes = 0;
	(void) rocprim::exclusive_scan(nullptr, tmp_bytes, m->d_sam_len.p, m->d_sam_off.p, 0u, (size_t) n + 1, rocprim::plus<uint32_t>(), m->st);
	if (m->d_scan_tmp.reserve(tmp_bytes + 16)) { ngm::pipeline_set_error("out of device memory (scan)"); return -12; }
	MAP_HIP_TRY(rocprim::exclusive_scan(m->d_scan_tmp.p, tmp_bytes, m->d_sam_len.p, m->d_sam_off.p, 0u, (size_t) n + 1, rocprim::plus<uint32_t>(), m->st));
	uint32_t total32 = 0;
	unsigned long long ctr[4] = {0, 0, 0, 0};
	MAP_HIP_TRY(hipMemcpyAsync(&total32, m->d_sam_off.p + n, 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(ctr, m->d_argos_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	if (ctr[3] != (unsigned long long) total32) {   // the 32-bit prefix sums have wrapped
		ngm::pipeline_set_error("ngm_mapper_map_argos: the text of this batch of %d reads is %llu bytes, beyond the 32-bit offsets of a batch: use smaller batches", n, ctr[3]);
		return -75;
	}
	const uint64_t total = total32;
	if (total > 0) {
		if (m->d_sam_text.reserve((size_t) total + 16)) { ngm::pipeline_set_error("out of device memory (argos text)"); return -12; }
		T.out = m->d_sam_text.p;
		hipLaunchKernelGGL(ngm::argos_write_kernel, dim3((n + 255) / 256), dim3(256), 0, m->st, T);
		MAP_HIP_TRY(hipGetLastError());
	}
	MAP_HIP_TRY(hipEventRecord(m->aev[3], m->st));
	m->sam_text_bytes = total;
	if (total > 0 && total <= out_cap && out) MAP_HIP_TRY(hipMemcpyAsync(out, m->d_sam_text.p, (size_t) total, hipMemcpyDeviceToHost, m->st));
	stage_txt.done_after(m->aev[3]);
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	m->argos_unknown += ctr[0];
	for (int c = 0; c < 3; ++c) m->argos_ctr[c] += cls_n[c];
	m->argos_ctr[3] += ctr[2];
	if (stats) { stats[0] = (uint64_t) n; stats[1] = ctr[1]; stats[2] = 0; }
	auto et = [](hipEvent_t a, hipEvent_t b) { float t = 0; return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.f; };
	if (kernel_ms) *kernel_ms = et(m->aev[0], m->aev[1]) + et(m->aev[2], m->aev[3]);
	m->ms[0] = m->cs_kernel_ms;
	m->ms[7] = et(m->ev[0], m->ev[1]);
	if (np > 0) { m->ms[1] = et(m->ev[1], m->ev[2]); m->ms[2] = et(m->ev[2], m->ev[3]); }
	return (long long) total;
}

int ngm_argos_prolog(const ngm_ref *ref, uint64_t total_reads, char *out, size_t cap) {
	// ScoreWriter::DoWriteProlog (ScoreWriter.cpp:19-35): "#<TotalSeqs>\n", then "#", "<i>:<name>\t" per contig, "\n"
	if (!ref) return -22;
	std::string s = "#" + std::to_string((unsigned) total_reads) + "\n#";
	for (size_t i = 0; i < ref->contigs.size(); ++i) s += std::to_string(i) + ":" + ref->contigs[i].name + "\t";
	s += "\n";
	if (s.size() > 0x7FFFFFFFu) return -75;
	if (out && s.size() <= cap) memcpy(out, s.data(), s.size());
	return (int) s.size();
}

int ngm_debug_argos_order(uint32_t n, const float *score, const uint32_t *rank, float min_score, int read_len, int match_bonus, uint32_t *order, uint32_t out[3]) {
	// what argos_order_kernel + the host's H sort do with one read (the device's filter, keys and classes restated on the host)
	if ((n && (!score || !order)) || !out) return -22;
	const bool filter = min_score > 0.f;
	const float min = !filter ? 0.f : min_score <= 1.0f ? ((float) read_len * (float) match_bonus) * min_score : min_score;
	std::vector<uint32_t> v;
	uint32_t npos = 0;
	for (uint32_t x = 0; x < n; ++x) if (!filter || score[x] >= min) { v.push_back(x); npos += score[x] > 0.f ? 1u : 0u; }
	auto key = [&](uint32_t x, uint32_t sec) { return ((uint64_t) ngm::argos_desc_key(score[x]) << 32) | sec; };
	std::sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return key(x, x) < key(y, y); });
	bool tie = false;
	for (uint32_t k = 0; k + 1 < npos; ++k) tie = tie || score[v[k]] == score[v[k + 1]];
	const uint32_t cls = !tie ? ngm::kArgosU : v.size() <= 16 ? ngm::kArgosS : ngm::kArgosH;
	if (cls == ngm::kArgosS && rank) {
		bool known = true;
		for (uint32_t c : v) known = known && rank[c] != ngm::kArgosRankUnknown;
		if (known) std::sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return key(x, rank[x]) < key(y, rank[y]); });
	} else if (cls == ngm::kArgosH) {
		(void) argos_sort_like_reference(v, score, rank);
	}
	std::copy(v.begin(), v.end(), order);
	out[0] = (uint32_t) v.size(); out[1] = npos; out[2] = cls;
	return 0;
}

int ngm_mapper_argos_counters(ngm_mapper *m, uint64_t out[4]) {
	if (!m || !out) return -22;
	for (int c = 0; c < 4; ++c) out[c] = m->argos_ctr[c];
	return 0;
}

int ngm_mapper_argos_path_counters(ngm_mapper *m, uint64_t out[2]) {
	if (!m || !out) return -22;
	out[0] = m->argos_long; out[1] = m->argos_unknown;
	return 0;
}

}  // extern "C"
