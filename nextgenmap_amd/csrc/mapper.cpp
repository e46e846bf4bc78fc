// mapper.cpp -- the device-resident mapping path above IAlignment (include/ngm_pipeline.h):
//   candidate search -> window gather -> BatchScore -> top-1 selection / MAPQ -> window gather -> BatchAlign.
// One ngm_mapper is what one NextGenMap CS thread owns (CS + ScoreBuffer + AlignmentBuffer + IAlignment,
// src/CS.cpp:455-461); everything between the read upload and the traceback download stays in HBM.
// This file: the mapper's life cycle, the C entry points, and map_impl -- one map call as a sequence of stages over one MapBatch
// (mapper_internal.h): begin -> search_and_score -> select -> align -> finish_hits -> write_sam -> kernel_times.  The select stage lives in
// mapper_select.cpp, the write_sam stage in mapper_sam.cpp, the candidate-search stage and the candidate-order replay in mapper_search.cpp.
// Every launch of a kernel of gather_device.h is here (the header's kernels are no templates: one translation unit).
#include "mapper_internal.h"
#include "align_device.h"
#include "gather_device.h"

using ngm::DevGuard;
using ngm::GpuStage;
using ngm::MapBatch;
using ngm::SamCall;
using ngm::parallel_for;
using ngm::run_cs;
using ngm::cs_host_arrays;

namespace ngm {
StageLock g_stage_lock[16][2];
std::atomic<long long> g_stage_hold_us[3], g_stage_wait_us[3];
}
using ngm::g_stage_hold_us;
using ngm::g_stage_wait_us;

namespace {

int upload_reads(ngm_mapper *m, int n, const char *reads) {
	const size_t bytes = (size_t) n * m->prm.qry_max_len;
	if (m->d_reads.reserve(bytes)) { ngm::pipeline_set_error("out of device memory (reads)"); return -12; }
	m->batch_reads = m->d_reads.p;
	MAP_HIP_TRY(hipMemcpyAsync(m->d_reads.p, reads, bytes, hipMemcpyHostToDevice, m->st));
	return 0;
}

// the host tail of a batch (CIGAR / MD strings, coordinate conversion) is embarrassingly parallel over reads;
// NextGenMap does it on its CS threads, here a batch is fanned out over the host cores
std::atomic<int> g_live_mappers{0};  // mapper instances share the host cores
// GPU stages (candidate search / score / align, each from its first launch to its stream sync) of the mapper instances of
// one process take turns: kernels of different instances then do not slow each other down, while the host stages of one
// instance still overlap the GPU stages of the others (NGM_HIP_GPU_STAGE_LOCK=0: let the streams share the GPU)
// NGM_HIP_GPU_STAGE_LOCK=2: one lock per stage KIND -- the align stage of one instance (1 wave per SIMD, hardly any LDS) may then
// run under the search stage of another (LDS-bound at 10 waves per CU), only stages of the same kind take turns.

char class_char(uint8_t c) {
	static const char t[8] = {'A', 'C', 'G', 'T', 'x', 'N', 0, 0};
	return t[c & 7];
}

// host twin of window_class (gather_device.h) for the CIGAR/MD pass: DecodeRefSequence into ASCII
void host_window(const ngm_ref *r, uint64_t offset, int buffer_len, int want, char *out) {
	const uint64_t concat_len = r->n_bases - 1;
	uint64_t len = (uint64_t) buffer_len - 2;
	if (offset >= concat_len) { memset(out, 'N', want); return; }
	uint64_t end = 0;
	if (offset + len > concat_len) { end = offset + len - concat_len; len -= end; }
	const uint64_t emitted = ((offset & 1) ? 1 : 0) + 2 * ((len + 1) / 2);
	for (int j = 0; j < want; ++j) {
		const uint64_t jj = (uint64_t) j;
		char ch;
		if (jj < emitted) ch = ((len & 1) && jj == emitted - 1) ? 'x' : class_char(r->host_cls[offset + jj]);
		else if (jj < emitted + end) ch = 'x';
		else ch = 0;
		out[j] = ch;
	}
}

// The two window geometries of a mapper (gather_device.h): the score stage's refMaxLen (ScoreBuffer.h:112), the align stage's
// (AlignmentBuffer.h:67: (qry_max_len + corridor) | 1 + 1)
ngm::WindowGeom window_geom(const ngm_mapper *m, bool align_stage) {
	const int q = m->prm.qry_max_len, c = m->prm.corridor;
	return ngm::WindowGeom{m->ref->n_bases - 1, align_stage ? ((q + c) | 2) : (((q + c) | 1) + 1), c >> 1};
}

// The gather's launch on the mapper's stream, shared by score_candidates, align and the test hook ngm_debug_gather_pairs: n_pairs pairs
// (pair_read, pair_loc, pair_sv in device memory) of the batch's reads into the engine's packed workspace (reserved by the caller)
int launch_gather(ngm_mapper *m, const ngm::WindowGeom &G, const uint32_t *pair_read, const uint32_t *pair_loc, const uint32_t *pair_sv, int n_pairs, int alt_dir) {
	ngm_hip_ctx *eng = m->eng;
	hipLaunchKernelGGL(ngm::gather_pairs_kernel, dim3((n_pairs + ngm::kSlots - 1) / ngm::kSlots), dim3(256), 0, m->st, m->batch_reads, m->d_read_len.p, m->prm.qry_max_len,
			m->ref->d_genome.p, G, pair_read, pair_loc, pair_sv, n_pairs, eng->RW, eng->FW, eng->packed.p, eng->lens.p, eng->blk_rows.p, alt_dir);
	MAP_HIP_TRY(hipGetLastError());
	return 0;
}

}  // namespace

namespace ngm {
// window gather + BatchScore of all np candidates of the batch (ScoreBuffer::DoRun, src/ScoreBuffer.cpp:80-130): d_scores[c] for every
// candidate; events ev[2] (behind the gather) and ev[3] (behind the score kernels).  The caller has reserved d_pair_read / d_scores and the
// engine's buffers for np candidates.
int score_candidates(ngm_mapper *m, int n, uint64_t np, int alt_dir) {
	ngm_hip_ctx *eng = m->eng;
	hipLaunchKernelGGL(ngm::expand_pairs_kernel, dim3((n + 255) / 256), dim3(256), 0, m->st, n, m->d_cand_base.p, m->d_cand_count.p, m->d_pair_read.p);
	if (int rc = launch_gather(m, window_geom(m, false), m->d_pair_read.p, m->d_out_loc.p, m->d_out_sv.p, (int) np, alt_dir)) return rc;
	MAP_HIP_TRY(hipEventRecord(m->ev[2], m->st));
	if (int rc = ngm::engine_score_packed(eng, m->prm.mode, (int) np, m->d_scores.p, m->st)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
	MAP_HIP_TRY(hipEventRecord(m->ev[3], m->st));
	return 0;
}
}  // namespace ngm

// The pair selection's launches on `st`, shared by search_and_score and the test hook ngm_debug_pair_select: pair_simple_kernel settles the pairs whose
// mates have one candidate each and -- with `choice_on_gpu` -- sorts the others into two lists, which the three instances of pair_choice_kernel
// (pair_device.h) then work through.  tied_n[4]: [0] tied pairs, [1] small pairs, [2] large pairs, [3] large pairs beyond kPairCap; list:
// 3 npairs + 2 words (small, large, huge); out: 2 npairs + 2 entries (small pairs from 0, large ones from npairs); tops: npairs + 1.
// The four of them may be null without choice_on_gpu.
static int launch_pair_select(hipStream_t st, size_t npairs, const uint32_t *cand_base, const uint32_t *cand_count, const float *scores, const uint32_t *loc,
		const uint16_t *read_len, int min_insert, int max_insert, float pair_score_cutoff, int32_t *mapq, int32_t *n_best, int32_t *info, bool choice_on_gpu,
		uint32_t *tied_n, uint32_t *list, ngm::PairOut *out, ngm::PairTop *tops) {
	const int min_d = min_insert, max_d = max_insert > 0 ? max_insert : INT_MAX;
	if (choice_on_gpu) MAP_HIP_TRY(hipMemsetAsync(tied_n, 0, 16, st));
	uint32_t *counts = choice_on_gpu ? tied_n + 1 : nullptr;
	hipLaunchKernelGGL(ngm::pair_simple_kernel, dim3((unsigned) ((npairs + 255) / 256)), dim3(256), 0, st, (int) npairs, cand_base, cand_count, scores, loc, read_len, min_d, max_d, mapq, n_best, info,
			list, list ? list + npairs : nullptr, counts);
	MAP_HIP_TRY(hipGetLastError());
	if (!choice_on_gpu) return 0;
	// persistent workgroups over the two lists (their lengths stay on the device); entries of the small pairs at out[0 ..), of the large
	// ones at out[npairs ..) (2^30 + ... in the numbering pair_simple_kernel puts into `info`)
	const float cutoff = pair_score_cutoff > 0 ? pair_score_cutoff : 0.9f;
	uint32_t *const huge_list = list + 2 * npairs, *const huge_count = tied_n + 3;   // entries of the large pairs with more than kPairCap candidates above the cut-off
	hipLaunchKernelGGL((ngm::pair_choice_kernel<64, 64>), dim3((unsigned) std::min<size_t>(npairs, 8192)), dim3(64), ngm::pair_choice_lds_bytes(64), st, (const uint32_t *) list, (const uint32_t *) counts,
			cand_base, cand_count, scores, loc, read_len, min_d, max_d, cutoff, out, tops, tied_n, (uint32_t) npairs, (uint32_t *) nullptr, (uint32_t *) nullptr, (const uint32_t *) nullptr);
	hipLaunchKernelGGL((ngm::pair_choice_kernel<ngm::kPairThreads, ngm::kPairCap>), dim3((unsigned) std::min<size_t>(npairs, 1024)), dim3(ngm::kPairThreads), ngm::pair_choice_lds_bytes(ngm::kPairCap), st,
			(const uint32_t *) (list + npairs), (const uint32_t *) (counts + 1), cand_base, cand_count, scores, loc, read_len, min_d, max_d, cutoff,
			out + npairs, tops, tied_n, (uint32_t) npairs, huge_list, huge_count, (const uint32_t *) nullptr);
	// ... and what outgrew those lists once more with kPairCapHuge of them (96 KB of LDS: one workgroup per CU; a few hundred pairs of repeat families per batch)
	static const bool huge_attr = [] { (void) hipFuncSetAttribute((const void *) ngm::pair_choice_kernel<1024, ngm::kPairCapHuge>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ngm::pair_choice_lds_bytes(ngm::kPairCapHuge)); return true; }();
	(void) huge_attr;
	hipLaunchKernelGGL((ngm::pair_choice_kernel<1024, ngm::kPairCapHuge>), dim3((unsigned) std::min<size_t>(npairs, 256)), dim3(1024), ngm::pair_choice_lds_bytes(ngm::kPairCapHuge), st,   // (one workgroup per CU either way: sixteen waves share a pair)
			(const uint32_t *) huge_list, (const uint32_t *) huge_count, cand_base, cand_count, scores, loc, read_len, min_d, max_d, cutoff,
			out + npairs, tops, tied_n, (uint32_t) npairs, (uint32_t *) nullptr, (uint32_t *) nullptr, (const uint32_t *) (list + npairs));
	MAP_HIP_TRY(hipGetLastError());
	return 0;
}

// The align stage's launches behind the gather (or the pack) wherever cigar_strings_kernel builds the strings -- every configuration but the affine
// personality's one finishing kernel -- on `st`, shared by align and the test hook ngm_debug_linear_strings: DP + traceback over the engine's packed
// workspace (engine_align_packed; with the engine's event [2] between the two), the runs compacted into runs_c with their total at *run_total, and
// with `S` CIGAR / MD / NM / identity per alignment, the strings in S->bytes with their total at *S->cursor.  ev_dp / ev_last: recorded behind the
// traceback / behind the last kernel when not null.  Buffers are the caller's: records 8 n, runs n * rs, runs_c n * rs, the two counters.
struct AlignStrings {
	ngm::CigarDevOut *out; char *bytes; unsigned long long capacity, *cursor;
	const uint16_t *read_len; const uint32_t *a_read;   // affine personality only: per read, and the read of alignment j
	int variant, hard_clip, silent_clip, alt_cigar;
};
static int launch_compact_runs(ngm_hip_ctx *eng, hipStream_t st, int n, int32_t *records, uint16_t *runs, int rs, uint16_t *runs_c, unsigned long long *run_total, bool traceback_first) {
	MAP_HIP_TRY(hipMemsetAsync(run_total, 0, 8, st));
	if (traceback_first) if (int rc = ngm::engine_affine_traceback_packed(eng, n, records, runs, rs, st)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
	hipLaunchKernelGGL(ngm::compact_runs_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, records, runs, rs, runs_c, run_total);
	MAP_HIP_TRY(hipGetLastError());
	return 0;
}
static int launch_align_strings(ngm_hip_ctx *eng, hipStream_t st, int mode, int n, int32_t *records, uint16_t *runs, int rs, uint16_t *runs_c, unsigned long long *run_total,
		const AlignStrings *S, hipEvent_t ev_dp, hipEvent_t ev_last) {
	const bool was_prof = eng->profiling;
	eng->profiling = true;  // brackets DP vs traceback with eng->ev[2]
	const int rc = ngm::engine_align_packed(eng, mode, n, records, runs, rs, st);
	eng->profiling = was_prof;
	if (rc) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
	if (ev_dp) MAP_HIP_TRY(hipEventRecord(ev_dp, st));
	if (int rc2 = launch_compact_runs(eng, st, n, records, runs, rs, runs_c, run_total, false)) return rc2;
	// CIGAR / MD / NM / identity on the GPU (cigar_device.h)
	if (S) {
		MAP_HIP_TRY(hipMemsetAsync(S->cursor, 0, 8, st));
		const int variant_cpu = S->variant == NGM_VARIANT_OCL_CPU ? 1 : 0;
		if (eng->prm.personality == NGM_PERSONALITY_AFFINE) hipLaunchKernelGGL(ngm::cigar_strings_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, st, n, records, runs_c, eng->packed.p, eng->RW, eng->FW,
				S->read_len, S->a_read, variant_cpu, S->hard_clip, S->silent_clip, S->out, S->bytes, S->capacity, S->cursor, 0);
		else hipLaunchKernelGGL(ngm::cigar_strings_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, st, n, records, runs_c, eng->packed.p, eng->RW, eng->FW,
				S->read_len, S->a_read, variant_cpu, S->hard_clip, S->silent_clip, S->out, S->bytes, S->capacity, S->cursor, S->alt_cigar);
		MAP_HIP_TRY(hipGetLastError());
	}
	if (ev_last) MAP_HIP_TRY(hipEventRecord(ev_last, st));
	return 0;
}

// ---- the stages of one map call (map_impl below), in their order; each returns 0 or the call's error code ---------------------------
namespace {

// (before anything else: a refused batch passes its paired-end turn on -- MapBatch's PairTurn -- and touches nothing)
int check_arguments(const MapBatch &b) {
	const ngm_mapper *m = b.m;
	const int n = b.n;
	const bool paired = b.paired;
	if (n < 0) return -22;
	if (paired && m->prm.topn > 1) { ngm::pipeline_set_error("Paired end mode with topn > 1 not yet supported."); return -38; }  // ScoreBuffer::topNPE
	if (paired && (n & 1)) { ngm::pipeline_set_error("paired-end batches need an even number of reads"); return -22; }
	return 0;
}

// What is sized by the number of candidates: the host's arrays, and with `device` the score stage's buffers; `count`: growth is counted in b.regrown
int reserve_for_candidates(MapBatch &b, uint64_t cnt, bool device, bool count) {
	ngm_mapper *m = b.m;
	ngm_hip_ctx *eng = m->eng;
	const bool paired = b.paired;
	uint64_t &regrown = b.regrown;
	auto grow = [&](auto &buf, size_t want) { if (count && buf.cap < want) ++regrown; return buf.reserve(want); };
	MAP_OOM_TRY(grow(m->p_loc, cnt + 1) || grow(m->p_sv, cnt + 1) || (paired && grow(m->p_scores, cnt + 1)), "out of pinned host memory");
	if (!device) return 0;
	MAP_OOM_TRY(grow(m->d_pair_read, cnt) || grow(m->d_scores, cnt), "out of device memory (score stage)");
	const size_t had = eng->packed.cap + eng->lens.cap + eng->blk_rows.cap;
	if (int rc = ngm::engine_reserve(eng, (int) cnt)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
	if (count && eng->packed.cap + eng->lens.cap + eng->blk_rows.cap != had) ++regrown;
	return 0;
}

// the batch's reads and SAM inputs on their way, everything the score stage needs from the host reserved
int begin(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n;
	const bool paired = b.paired;
	const char *reads = b.reads;
	const void *d_reads_ext = b.d_reads_ext;
	SamCall *sam = b.sam;
	const int q = b.q = m->prm.qry_max_len;
	b.c = m->prm.corridor;
	b.str_stride = (size_t) 4 * std::max(1, q);
	for (auto &x : m->ms) x = 0.f;
	m->order_ms = 0.f;

	// reads already in HBM: the stages read them where they are (no copy); otherwise upload
	if (d_reads_ext) m->batch_reads = (const uint8_t *) d_reads_ext;
	b.host_timing = getenv("NGM_HIP_HOST_TIMING") != nullptr;
	b.alt_cigar = m->prm.bs_mapping ? NGM_ALT_BISULFITE : (m->prm.slam_seq ? NGM_ALT_SLAMSEQ : NGM_ALT_NONE);
	b.alt_dir = b.alt_cigar ? (paired ? 2 : 1) : 0;   // the pairs' direction bits (gather_pairs_kernel): score tables, conversion rule
	b.tp0 = std::chrono::steady_clock::now();
	MAP_HIP_TRY(hipEventRecord(m->ev[0], m->st));
	if (!d_reads_ext) if (int rc = upload_reads(m, n, reads)) return rc;
	if (sam) {
		// what the SAM records need beyond the reads: qualities, names (travel while the search runs)
		if (!m->sam_ready || (!paired) != (!m->sam_opt.paired) || m->prm.topn > 1) { ngm::pipeline_set_error("ngm_mapper_map_sam: call ngm_mapper_set_sam_options first (single alignments only; paired as configured)"); return -22; }
		if ((unsigned long long) n * (unsigned long long) (2 * q + 1024) + sam->names_bytes >= 0xFFFFFFFFull) { ngm::pipeline_set_error("ngm_mapper_map_sam: the text of %d reads may exceed the 32-bit offsets of a batch: use smaller batches", n); return -75; }
		MAP_OOM_TRY(m->d_sam_quals.reserve((size_t) n * q) || m->d_sam_names.reserve(sam->names_bytes + 16) || m->d_sam_meta.reserve(n) || m->p_sam_hits.reserve(n) || m->p_sam_refs.reserve(n) ||
				m->d_sam_hits.reserve(n) || m->d_sam_refs.reserve(n), "out of memory (SAM stage)");
		MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_quals.p, sam->quals, (size_t) n * q, hipMemcpyHostToDevice, m->st));
		if (sam->names_bytes) MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_names.p, sam->names, sam->names_bytes, hipMemcpyHostToDevice, m->st));
		MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_meta.p, sam->meta, (size_t) n * sizeof(ngm::SamMeta), hipMemcpyHostToDevice, m->st));
		if (sam->polya && n > 0) {
			MAP_OOM_TRY(m->d_sam_polya.reserve((size_t) n), "out of memory (SAM stage)");
			MAP_HIP_TRY(hipMemcpyAsync(m->d_sam_polya.p, sam->polya, (size_t) n * sizeof(uint16_t), hipMemcpyHostToDevice, m->st));
		}
		b.hits = m->p_sam_hits.p;
	}
	// ---- in front of the search, outside the turn: everything the score stage needs from the host.  What is sized by the number of reads
	// is final here; what is sized by the number of candidates is reserved for a predicted count -- 5/4 of the most this mapper has seen,
	// at least one per read -- and once more for the real count behind the search's synchronisation: a no-op when it fits, a buffer that
	// grows inside the turn when it does not (the first batches of a run; counted in turn_dbg[2]).
	MAP_OOM_TRY(m->p_winner.reserve(n) || m->p_mapq.reserve(n) || m->p_nbest.reserve(n) || m->p_best.reserve(n), "out of pinned host memory");
	MAP_OOM_TRY(m->d_winner.reserve(n) || m->d_mapq.reserve(n) || m->d_nbest.reserve(n) || m->d_best.reserve(n), "out of device memory (score stage)");
	if (int rc = reserve_for_candidates(b, std::min<uint64_t>(std::max<uint64_t>((uint64_t) n, m->np_seen_max + m->np_seen_max / 4), 0x7FFFFFFFull), true, false)) return rc;
	b.h_winner = m->p_winner.p;
	b.h_mapq = m->p_mapq.p; b.h_nbest = m->p_nbest.p;
	b.h_best = m->p_best.p;
	b.pair_flags.assign(n, 0);
	return 0;
}

// the search + score turn's GPU work: candidate search, then all candidates of the batch in one BatchScore, top-1 selection, the pair
// selection's kernels, the downloads; returns behind the score stage's synchronisation (np == 0: behind the search's)
int search_and_score(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n;
	const bool paired = b.paired;
	GpuStage &stage_cs = b.stage_cs;
	m->cs_paired = paired;
	m->turn_dbg[2] = 0;
	if (int rc = run_cs(m, n, &stage_cs, true)) return rc;
	MAP_HIP_TRY(hipEventRecord(m->ev[1], m->st));
	const uint64_t np = b.np = m->n_cand;
	m->np_seen_max = std::max(m->np_seen_max, np);
	b.lap(0);
	if (const char *dump = getenv("NGM_HIP_DUMP_COUNTS")) {  // diagnostics: candidates per read, appended batch after batch
		if (int rc = cs_host_arrays(m)) return rc;
		if (FILE *f = fopen(dump, "ab")) { fwrite(m->h_count.data(), 4, (size_t) n, f); fclose(f); }
	}

	if (int rc = reserve_for_candidates(b, np, np > 0, true)) return rc;
	m->turn_dbg[2] = b.regrown;
	uint32_t *h_winner = b.h_winner, *h_loc = b.h_loc = m->p_loc.p, *h_sv = b.h_sv = m->p_sv.p;
	int32_t *h_mapq = b.h_mapq, *h_nbest = b.h_nbest;
	float *h_best = b.h_best, *h_scores = b.h_scores = m->p_scores.p;
	if (np == 0) { if (int rc = cs_host_arrays(m)) return rc; for (int i = 0; i < n; ++i) { h_winner[i] = 0xFFFFFFFFu; h_mapq[i] = 0; h_nbest[i] = 0; h_best[i] = 0.f; } }
	if (np == 0) return 0;
	// ---- score stage: all candidates of the batch in one BatchScore -------------------------------------
	// (its buffers: reserve_for_candidates above)
	stage_cs.acquire();
	if (int rc = ngm::score_candidates(m, n, np, b.alt_dir)) return rc;
	hipLaunchKernelGGL(ngm::select_top1_kernel, dim3((n + 255) / 256), dim3(256), 0, m->st, n, m->d_cand_base.p, m->d_cand_count.p,
			m->d_scores.p, m->d_out_loc.p, m->d_out_sv.p, m->d_winner.p, m->d_mapq.p, m->d_nbest.p, m->d_best.p);
	MAP_HIP_TRY(hipGetLastError());
	const bool pe_select = b.pe_select = paired && !m->fast_pairing;   // --fast-pairing: the mates are selected single-end, the writer checks the pair (AlignmentBuffer.cpp:176-199)
	const bool simple_on_gpu = b.simple_on_gpu = pe_select && m->prm.strata == 0;   // (--strata touches NH of every pair: host)
	// ... and the pairs with choices: everything the scores alone decide (pair_device.h); NGM_HIP_HOST_PAIR_CHOICE=1 keeps the host's walk
	// (which side walks the pairs with choices depends on the workload: with ~1.2 candidates per read -- a genome without a heavy tail --
	// the pairs with choices have two or three candidates, the host's pass 1 is 1.4 ms on the pool beside the other instance's kernels,
	// and the two extra kernel launches cost the step more than they save: 50.0-50.3 M reads/s against 51.8 M on one box,
	// profiles/r05_main_leg_ab_vs_r04.txt; from 3 candidates per read on the GPU takes them.  NGM_HIP_HOST_PAIR_CHOICE=1 / NGM_HIP_GPU_PAIR_CHOICE=1 force a side)
	static const bool pair_choice_host = getenv("NGM_HIP_HOST_PAIR_CHOICE") != nullptr, pair_choice_force = getenv("NGM_HIP_GPU_PAIR_CHOICE") != nullptr;
	const bool choice_on_gpu = b.choice_on_gpu = simple_on_gpu && !pair_choice_host && (pair_choice_force || np >= 3ull * (uint64_t) n);
	if (simple_on_gpu) {
		// pairs whose mates have one candidate each (most): settled here, the host only sums their insert sizes; the others are sorted
		// into two lists for pair_choice_kernel (mates with up to 64 candidates each: one wave per pair; the rest: a workgroup)
		const size_t npairs = (size_t) n / 2;
		MAP_OOM_TRY(m->d_pair_info.reserve(npairs + 1) || m->p_pair_info.reserve(npairs + 1), "out of memory (pair selection)");
		if (choice_on_gpu) {
			MAP_OOM_TRY(m->d_pair_out.reserve(2 * npairs + 2) || m->d_pair_top.reserve(npairs + 1) || m->d_pair_tied_n.reserve(4) || m->p_pair_tied_n.reserve(4) || m->d_pair_list.reserve(3 * npairs + 2),
					"out of memory (pair selection)");
		}
		if (int rc = launch_pair_select(m->st, npairs, m->d_cand_base.p, m->d_cand_count.p, m->d_scores.p, m->d_out_loc.p, m->d_read_len.p, m->prm.min_insert_size, m->prm.max_insert_size,
				m->prm.pair_score_cutoff, m->d_mapq.p, m->d_nbest.p, m->d_pair_info.p, choice_on_gpu, m->d_pair_tied_n.p, m->d_pair_list.p, m->d_pair_out.p, m->d_pair_top.p)) return rc;
		if (choice_on_gpu) {
			MAP_HIP_TRY(hipMemcpyAsync(m->p_pair_tied_n.p, m->d_pair_tied_n.p, 16, hipMemcpyDeviceToHost, m->st));
		}
		MAP_HIP_TRY(hipMemcpyAsync(m->p_pair_info.p, m->d_pair_info.p, (size_t) (n / 2) * 4, hipMemcpyDeviceToHost, m->st));
	}
	MAP_HIP_TRY(hipEventRecord(m->ev[4], m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_winner, m->d_winner.p, (size_t) n * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_mapq, m->d_mapq.p, (size_t) n * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_nbest, m->d_nbest.p, (size_t) n * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_best, m->d_best.p, (size_t) n * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_loc, m->d_out_loc.p, np * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(h_sv, m->d_out_sv.p, np * 4, hipMemcpyDeviceToHost, m->st));
	if (paired) MAP_HIP_TRY(hipMemcpyAsync(h_scores, m->d_scores.p, np * 4, hipMemcpyDeviceToHost, m->st));
	if (int rc = ngm::cs_enqueue_host_arrays(m)) return rc;   // the search's per-read arrays, deferred to here: they travel under the next instance's kernels
	stage_cs.done_after(m->ev[4]);
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	return 0;
}

// the align stage's lists: one entry per read that has a winner (topn > 1: per candidate to report), in read order
void compact_winners(MapBatch &b) {
	const int n = b.n, topn = b.topn;
	const uint32_t *h_winner = b.h_winner, *h_loc = b.h_loc, *h_sv = b.h_sv;
	const std::vector<uint32_t> &tn_pairs = b.tn_pairs;
	b.a_read.resize((size_t) n * topn); b.a_loc.resize((size_t) n * topn); b.a_sv.resize((size_t) n * topn); b.a_out.resize((size_t) n * topn); b.a_pair.resize((size_t) n * topn);
	std::vector<uint32_t> &a_read = b.a_read, &a_loc = b.a_loc, &a_sv = b.a_sv, &a_out = b.a_out, &a_pair = b.a_pair;
	int &na = b.na;
	if (topn == 1 || b.np == 0) {
		// winners, compacted in read order: count per slice, prefix, fill (the gathers through h_winner miss the caches)
		const int slices = std::max(1, std::min(256, n / 4096));
		std::vector<int> first(slices + 1, 0);
		parallel_for(slices, [&](int lo, int hi) {
			for (int s2 = lo; s2 < hi; ++s2) {
				const int i0 = (int) ((long long) n * s2 / slices), i1 = (int) ((long long) n * (s2 + 1) / slices);
				int cnt = 0;
				for (int i = i0; i < i1; ++i) cnt += h_winner[i] != 0xFFFFFFFFu;
				first[s2 + 1] = cnt;
			}
		}, 1);
		for (int s2 = 0; s2 < slices; ++s2) first[s2 + 1] += first[s2];
		na = first[slices];
		parallel_for(slices, [&](int lo, int hi) {
			for (int s2 = lo; s2 < hi; ++s2) {
				const int i0 = (int) ((long long) n * s2 / slices), i1 = (int) ((long long) n * (s2 + 1) / slices);
				int at = first[s2];
				for (int i = i0; i < i1; ++i) if (h_winner[i] != 0xFFFFFFFFu) {
					a_read[at] = (uint32_t) i; a_out[at] = (uint32_t) i; a_pair[at] = h_winner[i]; a_loc[at] = h_loc[h_winner[i]]; a_sv[at] = h_sv[h_winner[i]]; ++at;
				}
			}
		}, 1);
	} else {
		for (int i = 0; i < n; ++i) for (int t = 0; t < topn; ++t) {
			const uint32_t w = tn_pairs[(size_t) i * topn + t];
			if (w == 0xFFFFFFFFu) break;
			a_read[na] = i; a_out[na] = (uint32_t) (i * topn + t); a_pair[na] = w; a_loc[na] = h_loc[w]; a_sv[na] = h_sv[w]; ++na;
		}
	}
}

// the pieces both tails of the align stage are made of:
// the alignments' runs compacted into d_runs_c, their total at d_total[0] -- with the affine traceback kernels in front where the finishing
// kernel has left alignments to the host (trace matrix and end cells are still there)
int compact_runs(MapBatch &b, int rs, bool traceback_first) {
	ngm_mapper *m = b.m;
	const int na = b.na;
	MAP_OOM_TRY(m->d_runs_c.reserve((size_t) na * rs), "out of device memory (runs)");
	return launch_compact_runs(m->eng, m->st, na, m->d_records.p, m->d_runs.p, rs, m->d_runs_c.p, m->d_total.p, traceback_first);
}
// ... the compacted runs on the host (behind the synchronisation that brought their total)
int fetch_runs(MapBatch &b, unsigned long long n_runs_total) {
	ngm_mapper *m = b.m;
	MAP_OOM_TRY(m->p_runs.reserve(n_runs_total + 1), "out of pinned host memory");
	b.h_runs = m->p_runs.p;
	MAP_HIP_TRY(hipMemcpy(b.h_runs, m->d_runs_c.p, n_runs_total * 2, hipMemcpyDeviceToHost));
	return 0;
}
// ... and the device's string stream (the SAM stage reads it where it is)
int fetch_strings(MapBatch &b, unsigned long long n_str_total) {
	ngm_mapper *m = b.m;
	b.str_base = n_str_total;
	MAP_OOM_TRY(m->p_str.reserve(n_str_total + 1), "out of pinned host memory");
	if (n_str_total && !b.sam) MAP_HIP_TRY(hipMemcpy(m->p_str.p, m->d_str.p, n_str_total, hipMemcpyDeviceToHost));
	return 0;
}

// ---- alignment stage: one pair per read that has a winner (AlignmentBuffer::DoRun) --------------------
int align(MapBatch &b) {
	ngm_mapper *m = b.m;
	ngm_hip_ctx *eng = m->eng;
	const int q = b.q, c = b.c, mode = m->prm.mode, topn = b.topn, alt_cigar = b.alt_cigar, alt_dir = b.alt_dir;
	compact_winners(b);
	const int na = b.na;
	const int rs = ngm::run_stride(q, c);
	MAP_OOM_TRY(m->p_rec.reserve((size_t) na * 8 + 8), "out of pinned host memory");
	int32_t *h_rec = b.h_rec = m->p_rec.p;
	const ngm::WindowGeom Ga = window_geom(m, true);
	b.align_buf_len = Ga.buffer_len;
	static const bool dev_strings = !getenv("NGM_HIP_HOST_CIGAR");
	b.dev_strings = dev_strings;
	GpuStage stage_align(m, 1, false);
	if (na > 0) {
		MAP_OOM_TRY(m->d_a_read.reserve(na) || m->d_a_loc.reserve(na) || m->d_a_sv.reserve(na) || m->d_records.reserve((size_t) na * 8) ||
				m->d_runs.reserve((size_t) na * rs), "out of device memory (align stage)");
		if (int rc = ngm::engine_reserve(eng, na)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
		MAP_HIP_TRY(hipMemcpyAsync(m->d_a_read.p, b.a_read.data(), (size_t) na * 4, hipMemcpyHostToDevice, m->st));
		MAP_HIP_TRY(hipMemcpyAsync(m->d_a_loc.p, b.a_loc.data(), (size_t) na * 4, hipMemcpyHostToDevice, m->st));
		MAP_HIP_TRY(hipMemcpyAsync(m->d_a_sv.p, b.a_sv.data(), (size_t) na * 4, hipMemcpyHostToDevice, m->st));
		// (what the turn needs besides: the string buffers, and the finishing kernel's two counters cleared -- in front of the turn, not in it)
		static const bool tail_split = getenv("NGM_HIP_ALIGN_TAIL_SPLIT") != nullptr;
		const bool affine = m->prm.personality == NGM_PERSONALITY_AFFINE;
		const bool finish = affine && dev_strings && topn == 1 && !tail_split;
		const unsigned long long scap = (unsigned long long) na * 96ull + 4096ull;
		MAP_OOM_TRY(dev_strings && (m->d_cigout.reserve(na) || m->d_str.reserve(scap) || m->p_cigout.reserve(na)), "out of memory (CIGAR strings)");
		MAP_OOM_TRY(!finish && m->d_runs_c.reserve((size_t) na * rs), "out of device memory (runs)");
		if (finish) MAP_HIP_TRY(hipMemsetAsync(m->d_total.p + 8, 0, 16, m->st));   // the stage's one memset: stream cursor + fall-back counter
		MAP_HIP_TRY(hipStreamSynchronize(m->st));   // (the uploads travel outside the stage lock)
		stage_align.acquire();
		MAP_HIP_TRY(hipEventRecord(m->ev[5], m->st));
		if (int rc = launch_gather(m, Ga, m->d_a_read.p, m->d_a_loc.p, m->d_a_sv.p, na, alt_dir)) return rc;
		MAP_HIP_TRY(hipEventRecord(m->ev[6], m->st));
		// affine, strings on the GPU, one alignment per read: DP, then ONE finishing kernel from the trace matrix to the strings
		// (affine_finish_kernel, cigar_device.h).  NGM_HIP_ALIGN_TAIL_SPLIT=1 keeps the three kernels traceback / compact_runs / cigar_strings
		// and their downloads (tests); they also serve every other mode, and the alignments the finishing kernel leaves to the host.
		unsigned long long n_runs_total = 0, n_str_total = 0;
		if (finish) {
			unsigned long long ctr[2] = {0, 0};   // [0] bytes of the string stream, [1] alignments left to the host
			const ngm::AlignFinish fin{m->d_cigout.p, m->d_str.p, scap, m->d_total.p + 8};
			const bool was_prof = eng->profiling;
			eng->profiling = true;  // brackets DP vs finishing kernel with eng->ev[2]
			if (int rc = ngm::engine_align_packed(eng, mode, na, m->d_records.p, m->d_runs.p, rs, m->st, &fin)) { eng->profiling = was_prof; ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
			eng->profiling = was_prof;
			MAP_HIP_TRY(hipEventRecord(m->ev[7], m->st));
			MAP_HIP_TRY(hipEventRecord(m->ev[8], m->st));
			MAP_HIP_TRY(hipMemcpyAsync(m->p_cigout.p, m->d_cigout.p, (size_t) na * sizeof(ngm::CigarDevOut), hipMemcpyDeviceToHost, m->st));
			MAP_HIP_TRY(hipMemcpyAsync(ctr, m->d_total.p + 8, 16, hipMemcpyDeviceToHost, m->st));
			stage_align.done_after(m->ev[8]);
			MAP_HIP_TRY(hipStreamSynchronize(m->st));
			n_str_total = std::min<unsigned long long>(ctr[0], scap);
			if (int rc = fetch_strings(b, n_str_total)) return rc;
			if (ctr[1]) {
				// strings beyond the device's rows (rare): the old traceback on the same batch -- trace matrix and end cells are still there --
				// and the host's builder for exactly those alignments
				if (int rc = compact_runs(b, rs, true)) return rc;
				MAP_HIP_TRY(hipMemcpyAsync(h_rec, m->d_records.p, (size_t) na * 8 * 4, hipMemcpyDeviceToHost, m->st));
				MAP_HIP_TRY(hipMemcpyAsync(&n_runs_total, m->d_total.p, 8, hipMemcpyDeviceToHost, m->st));
				MAP_HIP_TRY(hipStreamSynchronize(m->st));
				if (int rc = fetch_runs(b, n_runs_total)) return rc;
			}
		} else {
			// DP + traceback, the runs compacted, and CIGAR / MD / NM / identity on the GPU (cigar_device.h); NGM_HIP_HOST_CIGAR=1 keeps the
			// host builders (tests).  ev[7] behind the traceback, ev[8] behind the stage's last kernel.
			const AlignStrings str{m->d_cigout.p, m->d_str.p, scap, m->d_total.p + 8, m->d_read_len.p, m->d_a_read.p, m->prm.variant, m->prm.hard_clip, m->prm.silent_clip, alt_cigar};
			if (int rc = launch_align_strings(eng, m->st, mode, na, m->d_records.p, m->d_runs.p, rs, m->d_runs_c.p, m->d_total.p, dev_strings ? &str : nullptr, m->ev[7], m->ev[8])) return rc;
			if (dev_strings) {
				MAP_HIP_TRY(hipMemcpyAsync(m->p_cigout.p, m->d_cigout.p, (size_t) na * sizeof(ngm::CigarDevOut), hipMemcpyDeviceToHost, m->st));
				MAP_HIP_TRY(hipMemcpyAsync(&n_str_total, m->d_total.p + 8, 8, hipMemcpyDeviceToHost, m->st));
			}
			MAP_HIP_TRY(hipMemcpyAsync(h_rec, m->d_records.p, (size_t) na * 8 * 4, hipMemcpyDeviceToHost, m->st));
			MAP_HIP_TRY(hipMemcpyAsync(&n_runs_total, m->d_total.p, 8, hipMemcpyDeviceToHost, m->st));
			stage_align.done_after(m->ev[8]);
			MAP_HIP_TRY(hipStreamSynchronize(m->st));
			if (int rc = fetch_runs(b, n_runs_total)) return rc;
			if (dev_strings) {
				n_str_total = std::min<unsigned long long>(n_str_total, scap);
				if (int rc = fetch_strings(b, n_str_total)) return rc;
			}
		}
	}
	stage_align.done();

	b.lap(3);
	return 0;
}

// ---- host: CIGAR / MD, final positions --------------------------------------------------------------
// (SAM stage: the strings stay in the device's byte stream and the records point into it; only strings the device could
// not build are made here and appended to that stream)
void finish_hits(MapBatch &b) {
	ngm_mapper *m = b.m;
	const ngm_ref *r = m->ref;
	const int n = b.n, q = b.q, c = b.c, topn = b.topn, na = b.na, alt_cigar = b.alt_cigar;
	const bool paired = b.paired;
	const char *reads = b.reads;
	ngm_hit *hits = b.hits;
	char *cigars = b.cigars, *mds = b.mds;
	const SamCall *sam = b.sam;
	const size_t str_stride = b.str_stride;
	const uint64_t str_base = b.str_base;
	const int32_t *h_mapq = b.h_mapq, *h_nbest = b.h_nbest, *h_rec = b.h_rec;
	const float *h_best = b.h_best, *h_scores = b.h_scores;
	const uint16_t *h_runs = b.h_runs;
	const std::vector<int> &pair_flags = b.pair_flags;
	const std::vector<uint32_t> &a_read = b.a_read, &a_loc = b.a_loc, &a_sv = b.a_sv, &a_out = b.a_out, &a_pair = b.a_pair;
	std::vector<char> &extra = b.extra;
	const int align_buf_len = b.align_buf_len;
	const bool dev_strings = b.dev_strings;
	ngm::SamRef *sam_refs = b.sam_refs = sam ? m->p_sam_refs.p : nullptr;
	std::mutex extra_mu;
	parallel_for(n, [&](int lo, int hi) {
		for (int i = lo; i < hi; ++i) for (int t = 0; t < topn; ++t) {
			const size_t o = (size_t) i * topn + t;
			ngm_hit &h = hits[o];
			memset(&h, 0, sizeof(h));
			h.n_candidates = (int) m->h_count[i];
			h.max_votes = m->h_maxv[i];
			h.mapq = h_mapq[i];
			h.n_best = h_nbest[i];
			h.score = h_best[i];
			h.pair_flags = pair_flags[i];
			if (!sam) { cigars[o * str_stride] = 0; mds[o * str_stride] = 0; }
			else sam_refs[o] = ngm::SamRef{0, 0, 0, 0};
		}
	});
	ngm::CigarParams cp{m->prm.match_bonus, -m->prm.mismatch_penalty, m->prm.variant, m->prm.hard_clip, m->prm.silent_clip, alt_cigar};
	parallel_for(na, [&](int lo, int hi) {
		std::vector<char> win((size_t) q + c + 8), qry((size_t) q + 8), scr(sam ? 2 * str_stride : 0);
		for (int j = lo; j < hi; ++j) {
			const int i = (int) a_read[j];
			const size_t o = a_out[j];
			ngm_hit &h = hits[o];
			if (topn > 1) h.score = h_scores[a_pair[j]];  // AS:i of this candidate
			const bool rev = a_sv[j] & 1u;
			h.reverse = rev;
			const char *rd = reads + (size_t) i * q;
			// (the read's length is only needed where the strings are built here: the rows of a batch -- 160 MB per million reads -- are
			// not touched on the host when the GPU has built CIGAR and MD)
			int L_cached = -1;
			auto read_length = [&]() { if (L_cached < 0) L_cached = (int) strnlen(rd, q); return L_cached; };
			ngm_hip_align_out ao{};
			ao.cigar = sam ? scr.data() : cigars + o * str_stride;
			ao.md = sam ? scr.data() + str_stride : mds + o * str_stride;
			bool host_strings = true;
			const ngm::CigarDevOut *dv = dev_strings ? &m->p_cigout.p[j] : nullptr;
			if (dv && (dv->flags & 1)) {  // built on the GPU: copy the two strings and the numbers
				if (!(dv->flags & 2)) { h.mapped = 0; continue; }  // no alignment could be built
				if (sam) { sam_refs[o] = ngm::SamRef{dv->cig_off, dv->md_off, dv->cig_len, dv->md_len}; host_strings = false; }
				else {
					memcpy(ao.cigar, m->p_str.p + dv->cig_off, dv->cig_len); ao.cigar[dv->cig_len] = 0;
					memcpy(ao.md, m->p_str.p + dv->md_off, dv->md_len); ao.md[dv->md_len] = 0;
				}
				ao.identity = dv->identity; ao.nm = dv->nm; ao.qstart = dv->qstart; ao.qend = dv->qend; ao.position_offset = dv->position_offset;
				ao.score_token = dv->score_token;
			} else if (m->prm.personality == NGM_PERSONALITY_AFFINE) {
				// matches / mismatches were counted by the traceback kernel: no window decode, no reverse complement here.
				// EndToEndAffine never touches pBuffer2: the SAM record carries AlignmentBuffer's "!!!" (AlignmentBuffer.cpp:109)
				ngm::build_cigar_affine(&h_rec[(size_t) j * 8], &h_runs[(size_t) (uint32_t) h_rec[(size_t) j * 8 + 6]], nullptr, nullptr, q, &ao, read_length());
				memcpy(ao.md, "!!!", 4);
			} else {
				const uint64_t offset = (uint64_t) a_loc[j] - (uint64_t) (c >> 1);
				host_window(r, offset, align_buf_len, q + c, win.data());
				memset(qry.data(), 0, qry.size());
				const int L = read_length();
				if (!rev) memcpy(qry.data(), rd, L);
				else for (int t = 0; t < L; ++t) {
					const char ch = rd[L - 1 - t];
					qry[t] = ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch;
				}
				const bool second = paired && (i & 1);
				ngm::build_cigar_md(cp, &h_rec[(size_t) j * 8], &h_runs[(size_t) (uint32_t) h_rec[(size_t) j * 8 + 6]], win.data(), qry.data(), &ao, cp.alt ? ((rev ? !second : second) ? 1 : 0) : 0);
				if (ao.score_token < 0) { h.mapped = 0; continue; }  // no alignment could be built
			}
			if (sam && host_strings) {
				const size_t cl = strlen(ao.cigar), ml = strlen(ao.md);
				std::lock_guard<std::mutex> lk(extra_mu);
				const size_t at = extra.size();
				extra.insert(extra.end(), ao.cigar, ao.cigar + cl);
				extra.insert(extra.end(), ao.md, ao.md + ml);
				sam_refs[o] = ngm::SamRef{(uint32_t) (str_base + at), (uint32_t) (str_base + at + cl), (uint16_t) cl, (uint16_t) ml};
			}
			h.identity = ao.identity; h.nm = ao.nm; h.qstart = ao.qstart; h.qend = ao.qend;
			// AlignmentBuffer.cpp:129 then SequenceProvider.convert (AlignmentBuffer.cpp:173)
			const uint64_t final_loc = (uint64_t) a_loc[j] + (uint64_t) (int64_t) ao.position_offset - (uint64_t) (c >> 1);
			int contig = 0; uint64_t cpos = 0;
			if (!ngm_ref_convert(r, final_loc, &contig, &cpos)) { h.mapped = 0; continue; }
			h.mapped = 1; h.contig = contig; h.pos = cpos;
		}
	});

	b.lap(4);
}

void kernel_times(MapBatch &b) {
	ngm_mapper *m = b.m;
	ngm_hip_ctx *eng = m->eng;
	const double *t_stage = b.t_stage;
	if (b.host_timing)
		fprintf(stderr, "[ngm-hip] host wall ms: candidate search %.1f | score stage + downloads %.1f | pair selection %.1f | align stage + downloads %.1f | CIGAR/positions %.1f\n",
				t_stage[0], t_stage[1], t_stage[2], t_stage[3], t_stage[4]);
	// kernel times
	auto et = [&](int a, int b) { float t = 0; if (hipEventElapsedTime(&t, m->ev[a], m->ev[b]) != hipSuccess) t = 0; return t; };
	m->ms[0] = m->cs_kernel_ms;  // sum of the candidate-search kernel launches only
	m->ms[7] = et(0, 1);          // ... and the whole CS stage including the host round trips between passes
	if (b.np > 0) { m->ms[1] = et(1, 2); m->ms[2] = et(2, 3); m->ms[3] = et(3, 4); }
	if (b.na > 0) {
		m->ms[4] = et(5, 6);
		float t = 0;
		if (hipEventElapsedTime(&t, m->ev[6], eng->ev[2]) == hipSuccess) m->ms[5] = t;
		if (hipEventElapsedTime(&t, eng->ev[2], m->ev[7]) == hipSuccess) m->ms[6] = t;
	}
}

// One map call: every mapping entry point comes through here.
int map_impl(ngm_mapper *m, int n, const char *reads, const void *d_reads_ext, ngm_hit *hits, char *cigars, char *mds, bool paired, SamCall *sam = nullptr) {
	if (!m) return -22;
	// (b owns the paired-end turn: passed on when b goes, on EVERY return from here on)
	MapBatch b(m, n, reads, d_reads_ext, hits, cigars, mds, paired, sam);
	if (int rc = check_arguments(b)) return rc;
	if (n == 0) return 0;
	DevGuard g(m->ref->device);
	if (int rc = begin(b)) return rc;
	if (int rc = search_and_score(b)) return rc;
	if (int rc = ngm::select(b)) return rc;
	if (int rc = align(b)) return rc;
	finish_hits(b);
	if (sam) if (int rc = ngm::write_sam(b)) return rc;
	kernel_times(b);
	return n;
}

}  // namespace

extern "C" {

int ngm_ref_decode(const ngm_ref *r, uint64_t offset, int buffer_len, char *out) {
	// runs the device window function over one window so that tests exercise the HBM copy
	DevGuard g(r->device);
	if (buffer_len < 2) return -22;
	const uint64_t concat_len = r->n_bases - 1;
	if (offset >= concat_len) { memset(out, 0, buffer_len); return 0; }  // DecodeRefSequence returns false
	// reuse the gather kernel: one pair, read of length 0, corridor 0, q = buffer_len rounded up
	const int q = 8, c = buffer_len;  // window = q + c >= buffer_len bytes
	const int RW = ngm::read_words(q), FW = (q + c + 7) / 8 + 1;
	ngm::Buf<uint32_t> d_out, d_pr, d_pl, d_ps;
	ngm::Buf<uint16_t> d_lens, d_rows, d_rl;
	ngm::Buf<uint8_t> d_reads;
	NGM_MEM_TRY(d_out.alloc((size_t) (RW + FW) * 64) || d_lens.alloc(64) || d_rows.alloc(4) || d_rl.alloc(4) || d_reads.alloc(q) || d_pr.alloc(1) || d_pl.alloc(1) || d_ps.alloc(1));
	MAP_HIP_TRY(hipMemset(d_rl.p, 0, 8)); MAP_HIP_TRY(hipMemset(d_reads.p, 0, q)); MAP_HIP_TRY(hipMemset(d_pr.p, 0, 4)); MAP_HIP_TRY(hipMemset(d_ps.p, 0, 4));
	const uint32_t loc = (uint32_t) offset;
	MAP_HIP_TRY(hipMemcpy(d_pl.p, &loc, 4, hipMemcpyHostToDevice));
	ngm::WindowGeom G{concat_len, buffer_len, 0};
	hipLaunchKernelGGL(ngm::gather_pairs_kernel, dim3(1), dim3(256), 0, 0, d_reads.p, d_rl.p, q, r->d_genome.p, G, d_pr.p, d_pl.p, d_ps.p, 1, RW, FW, d_out.p, d_lens.p, d_rows.p);
	MAP_HIP_TRY(hipGetLastError());
	std::vector<uint32_t> h((size_t) (RW + FW) * 64);
	MAP_HIP_TRY(hipMemcpy(h.data(), d_out.p, h.size() * 4, hipMemcpyDeviceToHost));
	for (int j = 0; j < buffer_len; ++j) {
		const uint32_t w = h[(size_t) (RW + j / 8) * 64];
		const int b = j & 7;
		const uint32_t cls = (b < 4) ? (w >> (8 * b)) & 15u : (w >> (8 * (b - 4) + 4)) & 15u;
		out[j] = class_char((uint8_t) cls);
	}
	return 1;
}

ngm_mapper *ngm_mapper_create(const ngm_ref *ref, const ngm_mapper_params *p) {
	if (!ref || !p) { ngm::pipeline_set_error("ngm_mapper_create: null argument"); return nullptr; }
	DevGuard g(ref->device);
	if (p->qry_max_len < ref->prm.kmer + 1 || p->qry_max_len > 1024) { ngm::pipeline_set_error("ngm_mapper_create: qry_max_len %d out of range", p->qry_max_len); return nullptr; }
	{
		// Every vote table of the search keeps a bin's forward and reverse votes in 16-bit halves of one word (cs_device.h).  A read of up
		// to qry_max_len - 1 bases has qry_max_len - k k-mers; the hits of one list for one (bin, strand) lie within 2^bin_size genome
		// positions, and a k-mer with max_kfreq hits or more is not voted (CS.cpp:122).  Two occurrences of a k-mer that is no homopolymer
		// are two positions apart or more: 2^(bin_size - 1) hits per list and bin.  A homopolymer's k-mer is stored twice per run and once
		// per bin border (PrefixTable.cpp:641-709), with k + 1 positions or more between two runs: up to 3 hits among 4 positions, so the
		// half is no bound for narrow bins -- but it is one from 128 positions on (2 * ceil(128 / 5) + 1 = 53 <= 64 at k = 4), and with at
		// most 1 020 k-mers per read the product passes 65 535 only at --bin-size 8, where the half is 128.  So the test below is exact
		// where it refuses: bins of 256 bases with 512 k-mers or more per read (an AC repeat gets there).  There a count would carry into
		// the other strand's half: refuse it here and not there.
		const long max_kfreq = p->max_kfreq > 0 ? p->max_kfreq : ref->auto_max_kfreq;
		const long per_kmer = std::min<long>(std::max<long>(1, max_kfreq - 1), std::max<long>(1, (1l << ref->prm.bin_size) >> 1));
		const long votes = (long) (p->qry_max_len - ref->prm.kmer) * per_kmer;
		if (votes > 65535) {
			ngm::pipeline_set_error("ngm_mapper_create: reads of up to %d bases with --bin-size %d and --max-kfreq %ld could collect %ld votes in one bin, and the search counts up to 65535 votes: use a smaller --bin-size",
									p->qry_max_len - 1, ref->prm.bin_size, max_kfreq, votes);
			return nullptr;
		}
	}
	ngm_hip_params ep{};
	ep.abi_version = NGM_HIP_ABI_VERSION;
	ep.qry_max_len = p->qry_max_len; ep.corridor = p->corridor;
	ep.match_bonus = p->match_bonus; ep.mismatch_penalty = p->mismatch_penalty; ep.gap_read_penalty = p->gap_read_penalty; ep.gap_ref_penalty = p->gap_ref_penalty;
	ep.variant = p->variant; ep.hard_clip = p->hard_clip; ep.silent_clip = p->silent_clip; ep.max_batch = 0;
	ep.personality = p->personality; ep.gap_extend_penalty = p->gap_extend_penalty;
	if (p->bs_mapping) {
		if (ref->prm.kmer_skip != 0) { ngm::pipeline_set_error("ngm_mapper_create: bisulfite mapping needs a reference index built with kmer_skip 0 (src/PrefixTable.cpp:199-207)"); return nullptr; }
		if (p->mode != 0) { ngm::pipeline_set_error("ngm_mapper_create: '--bs-mapping' and '--end-to-end' can't be used at the same time"); return nullptr; }   // Config.cpp:448-470 (-n is allowed there: ScoreBuffer::topNSE)
		ep.alt_scoring = ep.alt_cigar = NGM_ALT_BISULFITE; ep.match_bonus_tt = p->match_bonus_tt; ep.match_bonus_tc = p->match_bonus_tc;
	}
	if (p->slam_seq) {
		if (p->bs_mapping) { ngm::pipeline_set_error("ngm_mapper_create: '--bs-mapping' and '--slam-seq' can't be used at the same time!"); return nullptr; }  // Config.cpp:454-457
		if (p->personality != NGM_PERSONALITY_LINEAR) { ngm::pipeline_set_error("ngm_mapper_create: '--slam-seq' needs the default (linear-gap) personality: EndToEndAffine produces no per-base records (Align::ExtendedData)"); return nullptr; }
		ep.alt_cigar = NGM_ALT_SLAMSEQ;
		if (p->slam_seq & 2) { ep.alt_scoring = NGM_ALT_SLAMSEQ; ep.match_bonus_tt = p->match_bonus_tt; ep.match_bonus_tc = p->match_bonus_tc; }
	}
	ngm_hip_ctx *eng = ngm_hip_create(ref->device, &ep);
	if (!eng) { ngm::pipeline_set_error("%s", ngm_hip_last_error(nullptr)); return nullptr; }
	ngm_mapper *m = new ngm_mapper();
	++g_live_mappers;
	m->ref = ref; m->prm = *p; m->eng = eng; m->st = eng->stream;
	{
		int lo = 0, hi = 0;
		(void) hipDeviceGetStreamPriorityRange(&lo, &hi);  // hi = numerically smallest = greatest priority
		// (the order replay's stream: greatest priority -- persistent search workgroups hold every CU until their launch ends, and the replay
		// gets in as they leave)
		if (hipStreamCreateWithPriority(&m->st_hi, hipStreamNonBlocking, hi) != hipSuccess) m->st_hi = nullptr;
	}
	m->max_kfreq = p->max_kfreq > 0 ? p->max_kfreq : ref->auto_max_kfreq;
	for (auto &e : m->ev) (void) hipEventCreate(&e);
	for (auto &e : m->cev) (void) hipEventCreate(&e);
	for (auto &e : m->oev) (void) hipEventCreate(&e);
	if (const char *e = getenv("NGM_HIP_CS_EAGER_ARRAYS")) m->cs_eager_arrays = atoi(e) != 0;   // read per mapper: one process may hold one of each kind
	if (ngm::cs_configure(m, p) != 0) { ngm_mapper_destroy(m); return nullptr; }
	return m;
}

void ngm_mapper_destroy(ngm_mapper *m) {
	if (!m) return;
	if (--g_live_mappers == 0 && getenv("NGM_HIP_HOST_TIMING"))
		fprintf(stderr, "[ngm-hip] GPU stage lock, ms summed over all mappers: search + score held %.1f (waited %.1f) | align held %.1f (waited %.1f) | SAM text held %.1f (waited %.1f)\n",
				g_stage_hold_us[0] / 1e3, g_stage_wait_us[0] / 1e3, g_stage_hold_us[1] / 1e3, g_stage_wait_us[1] / 1e3, g_stage_hold_us[2] / 1e3, g_stage_wait_us[2] / 1e3);
	DevGuard g(m->ref->device);
	(void) hipStreamSynchronize(m->st);
	ngm_bgzf_destroy(m->bz);
	if (m->st_hi) { (void) hipStreamSynchronize(m->st_hi); (void) hipStreamDestroy(m->st_hi); }
	for (auto &e : m->ev) if (e) (void) hipEventDestroy(e);
	for (auto &e : m->cev) if (e) (void) hipEventDestroy(e);
	for (auto &e : m->oev) if (e) (void) hipEventDestroy(e);
	for (auto &e : m->aev) if (e) (void) hipEventDestroy(e);
	ngm_hip_destroy(m->eng);
	delete m;
}

int ngm_mapper_cs(ngm_mapper *m, int n, const char *reads, uint32_t *cand_offsets, float *max_votes) {
	if (!m || n < 0) return -22;
	DevGuard g(m->ref->device);
	if (n == 0) { cand_offsets[0] = 0; m->n_reads = 0; m->n_cand = 0; return 0; }
	if (int r = upload_reads(m, n, reads)) return r;
	m->cs_paired = false;
	if (int r = run_cs(m, n)) return r;
	if (int r = cs_host_arrays(m)) return r;
	uint32_t acc = 0;
	for (int i = 0; i < n; ++i) { cand_offsets[i] = acc; acc += m->h_count[i]; max_votes[i] = m->h_maxv[i]; }
	cand_offsets[n] = acc;
	return 0;
}

int ngm_mapper_cs_fetch(ngm_mapper *m, uint64_t *loc, uint8_t *strand, float *votes) {
	if (!m) return -22;
	DevGuard g(m->ref->device);
	if (m->n_cand == 0) return 0;
	std::vector<uint32_t> hl(m->n_cand), hs(m->n_cand);
	MAP_HIP_TRY(hipMemcpy(hl.data(), m->d_out_loc.p, m->n_cand * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(hs.data(), m->d_out_sv.p, m->n_cand * 4, hipMemcpyDeviceToHost));
	size_t w = 0;
	std::vector<uint32_t> order;
	for (int i = 0; i < m->n_reads; ++i) {
		const uint32_t b = m->h_base[i], c = m->h_count[i];
		order.resize(c);
		std::iota(order.begin(), order.end(), b);
		std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
			const uint64_t kx = ((uint64_t) hl[x] << 1) | (hs[x] & 1), ky = ((uint64_t) hl[y] << 1) | (hs[y] & 1);
			return kx < ky;
		});
		for (uint32_t j : order) { loc[w] = hl[j]; strand[w] = (uint8_t) (hs[j] & 1); votes[w] = (float) (hs[j] >> 1); ++w; }
	}
	return 0;
}

int ngm_mapper_map_se(ngm_mapper *m, int n, const char *reads, ngm_hit *hits, char *cigars, char *mds) {
	return map_impl(m, n, reads, nullptr, hits, cigars, mds, false);
}
int ngm_mapper_map_se_resident(ngm_mapper *m, int n, const char *reads, const void *d_reads_ext, ngm_hit *hits, char *cigars, char *mds) {
	return map_impl(m, n, reads, d_reads_ext, hits, cigars, mds, false);
}
int ngm_mapper_map_pe(ngm_mapper *m, int n, const char *reads, ngm_hit *hits, char *cigars, char *mds) {
	return map_impl(m, n, reads, nullptr, hits, cigars, mds, true);
}
int ngm_mapper_map_pe_resident(ngm_mapper *m, int n, const char *reads, const void *d_reads_ext, ngm_hit *hits, char *cigars, char *mds) {
	return map_impl(m, n, reads, d_reads_ext, hits, cigars, mds, true);
}

static_assert(sizeof(ngm_sam_read) == sizeof(ngm::SamMeta) && sizeof(ngm_sam_read) == 8, "ngm_sam_read is the device's per-read record");

long long ngm_mapper_map_sam(ngm_mapper *m, int n, const char *reads, const char *quals, const char *names, size_t names_bytes, const ngm_sam_read *meta,
		char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms) {
	return ngm_mapper_map_sam_trimmed(m, n, reads, quals, names, names_bytes, meta, nullptr, out, out_cap, stats, kernel_ms);
}

long long ngm_mapper_map_sam_trimmed(ngm_mapper *m, int n, const char *reads, const char *quals, const char *names, size_t names_bytes, const ngm_sam_read *meta,
		const uint16_t *polya_trimmed, char *out, size_t out_cap, uint64_t stats[3], float *kernel_ms) {
	if (!m || n < 0 || (n > 0 && (!reads || !quals || !meta))) return -22;
	SamCall sc{quals, names, names_bytes, reinterpret_cast<const ngm::SamMeta *>(meta), polya_trimmed, out, out_cap, stats, 0, 0.f};
	m->argos_text = false;
	const int rc = map_impl(m, n, reads, nullptr, nullptr, nullptr, nullptr, m->sam_opt.paired != 0, &sc);
	if (rc < 0) return rc;
	if (kernel_ms) *kernel_ms = sc.kernel_ms;
	if (n == 0 && stats) stats[0] = stats[1] = stats[2] = 0;
	return sc.text_bytes;
}

ngm_pair_state *ngm_pair_state_create(void) { return new ngm_pair_state(); }
void ngm_pair_state_destroy(ngm_pair_state *ps) { delete ps; }
int ngm_mapper_set_pair_state(ngm_mapper *m, ngm_pair_state *ps) { if (!m) return -22; m->ps = ps; return 0; }
int ngm_mapper_set_batch_seq(ngm_mapper *m, uint64_t seq) { if (!m) return -22; m->batch_seq = seq; return 0; }
int ngm_mapper_set_fast_pairing(ngm_mapper *m, int on) { if (!m) return -22; m->fast_pairing = on ? 1 : 0; return 0; }
int ngm_mapper_set_bam_sorter(ngm_mapper *m, ngm_bam_sort *s) { if (!m) return -22; m->sorter = s; return 0; }
int ngm_mapper_set_coverage(ngm_mapper *m, ngm_coverage *c) { if (!m) return -22; m->coverage = c; return 0; }
int ngm_mapper_set_snp(ngm_mapper *m, ngm_snp *s) { if (!m) return -22; m->snp = s; return 0; }
int ngm_mapper_set_count(ngm_mapper *m, ngm_count *c) { if (!m) return -22; m->count = c; return 0; }
int ngm_mapper_set_methyl(ngm_mapper *m, ngm_methyl *c) { if (!m) return -22; m->methyl = c; return 0; }

void *ngm_host_alloc(size_t bytes) {
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { ngm::pipeline_set_error("out of pinned host memory (%zu bytes)", bytes); return nullptr; }
	return p;
}
void ngm_host_free(void *p) { if (p) (void) hipHostFree(p); }

int ngm_debug_live_memory(uint64_t out[4]) {
	if (!out) return -22;
	const ngm::MemCount &d = ngm::DeviceMem::count, &h = ngm::PinnedMem::count;
	out[0] = d.live.load(std::memory_order_relaxed); out[1] = h.live.load(std::memory_order_relaxed);
	out[2] = d.calls.load(std::memory_order_relaxed); out[3] = h.calls.load(std::memory_order_relaxed);
	return 0;
}

int ngm_host_pin_to_device_node(int device) {
	char bdf[64] = {0};
	if (hipDeviceGetPCIBusId(bdf, (int) sizeof(bdf), device) != hipSuccess) { ngm::pipeline_set_error("no PCI bus id for device %d", device); return -19; }
	for (char *c = bdf; *c; ++c) *c = (char) tolower((unsigned char) *c);
	char path[256], line[4096] = {0};
	snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
	int node = -1;
	if (FILE *f = fopen(path, "r")) { if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f); }
	if (node < 0) return 0;
	snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
	FILE *f = fopen(path, "r");
	if (!f) return 0;
	const bool got = fgets(line, sizeof(line), f) != nullptr;
	fclose(f);
	if (!got) return 0;
	cpu_set_t set;
	CPU_ZERO(&set);
	int n = 0;
	for (const char *c = line; *c;) {  // "0-63,128-191"
		char *end = nullptr;
		const long a = strtol(c, &end, 10);
		if (end == c) break;
		long b = a;
		c = end;
		if (*c == '-') { b = strtol(c + 1, &end, 10); if (end == c + 1) break; c = end; }
		for (long x = a; x <= b && x < CPU_SETSIZE; ++x) if (x >= 0) { CPU_SET((int) x, &set); ++n; }
		if (*c == ',') ++c; else break;
	}
	if (n == 0) return 0;
	if (sched_setaffinity(0, sizeof(set), &set) != 0) return 0;  // (a container may forbid it: not an error)
	return n;
}

int ngm_mapper_cs_max_combined(ngm_mapper *m, float *out) {
	if (!m) return -22;
	DevGuard g(m->ref->device);
	if (m->n_reads > 0) MAP_HIP_TRY(hipMemcpy(out, m->d_max_both.p, (size_t) m->n_reads * 4, hipMemcpyDeviceToHost));
	return 0;
}

int ngm_mapper_set_reference_cs_batch(ngm_mapper *m, int reads) {
	if (!m || reads < 0) return -22;
	m->ref_cs_batch = reads & ~1;
	return 0;
}

int ngm_mapper_set_reference_score_buffer(ngm_mapper *m, int entries) {
	if (!m || entries < 0) return -22;
	m->ref_score_buffer = entries;
	return 0;
}

int ngm_mapper_lost_pairs(ngm_mapper *m, uint64_t *out) {
	if (!m || !out) return -22;
	*out = m->lost_pairs;
	return 0;
}

int ngm_mapper_path_counters(ngm_mapper *m, uint64_t out[8]) {
	if (!m || !out) return -22;
	out[0] = m->st_reads; out[1] = m->st_cands; out[2] = m->st_exact_lds; out[3] = m->st_exact_global;
	out[4] = m->st_order_reads; out[5] = m->st_order_big; out[6] = m->st_order_unknown; out[7] = m->st_heavy;
	return 0;
}

int ngm_debug_select_top1(int device, int n_reads, const uint32_t *base, const uint32_t *count, uint64_t n_cand, const float *scores, const uint32_t *loc,
		const uint32_t *strand_votes, uint32_t *winner, int32_t *mapq, int32_t *n_best, float *best_score) {
	if (n_reads <= 0 || !base || !count || !winner || !mapq || !n_best || !best_score) return -22;
	DevGuard g(device);
	ngm::DevBuf<uint32_t> d_base, d_count, d_loc, d_sv, d_win;
	ngm::DevBuf<int32_t> d_mq, d_nb;
	ngm::DevBuf<float> d_sc, d_best;
	const size_t nc = (size_t) std::max<uint64_t>(n_cand, 1);
	if (d_base.reserve(n_reads) || d_count.reserve(n_reads) || d_loc.reserve(nc) || d_sv.reserve(nc) || d_sc.reserve(nc) || d_win.reserve(n_reads) || d_mq.reserve(n_reads) ||
			d_nb.reserve(n_reads) || d_best.reserve(n_reads)) { ngm::pipeline_set_error("out of device memory (ngm_debug_select_top1)"); return -12; }
	MAP_HIP_TRY(hipMemcpy(d_base.p, base, (size_t) n_reads * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_count.p, count, (size_t) n_reads * 4, hipMemcpyHostToDevice));
	if (n_cand) {
		MAP_HIP_TRY(hipMemcpy(d_sc.p, scores, (size_t) n_cand * 4, hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_loc.p, loc, (size_t) n_cand * 4, hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_sv.p, strand_votes, (size_t) n_cand * 4, hipMemcpyHostToDevice));
	}
	hipLaunchKernelGGL(ngm::select_top1_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, 0, n_reads, d_base.p, d_count.p, d_sc.p, d_loc.p, d_sv.p, d_win.p, d_mq.p, d_nb.p, d_best.p);
	MAP_HIP_TRY(hipGetLastError());
	MAP_HIP_TRY(hipDeviceSynchronize());
	MAP_HIP_TRY(hipMemcpy(winner, d_win.p, (size_t) n_reads * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(mapq, d_mq.p, (size_t) n_reads * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(n_best, d_nb.p, (size_t) n_reads * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(best_score, d_best.p, (size_t) n_reads * 4, hipMemcpyDeviceToHost));
	return 0;
}

int ngm_debug_expand_pairs(int device, int n_reads, const uint32_t *base, const uint32_t *count, uint64_t n_cand, uint32_t *out) {
	if (n_reads <= 0 || !base || !count || (n_cand && !out)) return -22;
	DevGuard g(device);
	ngm::DevBuf<uint32_t> d_base, d_count, d_out;
	if (d_base.reserve(n_reads) || d_count.reserve(n_reads) || d_out.reserve((size_t) std::max<uint64_t>(n_cand, 1))) { ngm::pipeline_set_error("out of device memory (ngm_debug_expand_pairs)"); return -12; }
	MAP_HIP_TRY(hipMemcpy(d_base.p, base, (size_t) n_reads * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_count.p, count, (size_t) n_reads * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemset(d_out.p, 0xFF, (size_t) std::max<uint64_t>(n_cand, 1) * 4));
	hipLaunchKernelGGL(ngm::expand_pairs_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, 0, n_reads, d_base.p, d_count.p, d_out.p);
	MAP_HIP_TRY(hipGetLastError());
	MAP_HIP_TRY(hipDeviceSynchronize());
	if (n_cand) MAP_HIP_TRY(hipMemcpy(out, d_out.p, (size_t) n_cand * 4, hipMemcpyDeviceToHost));
	return 0;
}

int ngm_debug_pair_select(int device, int n_pairs, const uint32_t *base, const uint32_t *count, uint64_t n_cand, const float *scores, const uint32_t *loc,
		const uint16_t *read_len, int min_insert, int max_insert, float cutoff, int32_t *info, int32_t *mapq, int32_t *n_best, uint32_t counts[4], void *entries, void *tops) {
	if (n_pairs <= 0 || !base || !count || !read_len || !info || !mapq || !n_best || !counts || !entries || !tops || (n_cand && (!scores || !loc))) return -22;
	const size_t npairs = (size_t) n_pairs, n = 2 * npairs, nc = (size_t) std::max<uint64_t>(n_cand, 1);
	for (size_t i = 0; i < n; ++i) if ((uint64_t) base[i] + count[i] > n_cand) { ngm::pipeline_set_error("ngm_debug_pair_select: read %zu owns candidates beyond n_cand", i); return -22; }
	DevGuard g(device);
	ngm::DevBuf<uint32_t> d_base, d_count, d_loc, d_tied_n, d_list;
	ngm::DevBuf<uint16_t> d_len;
	ngm::DevBuf<float> d_sc;
	ngm::DevBuf<int32_t> d_mq, d_nb, d_info;
	ngm::DevBuf<ngm::PairOut> d_out;
	ngm::DevBuf<ngm::PairTop> d_top;
	if (d_base.reserve(n) || d_count.reserve(n) || d_len.reserve(n) || d_loc.reserve(nc) || d_sc.reserve(nc) || d_mq.reserve(n) || d_nb.reserve(n) || d_info.reserve(npairs + 1) ||
			d_tied_n.reserve(4) || d_list.reserve(3 * npairs + 2) || d_out.reserve(2 * npairs + 2) || d_top.reserve(npairs + 1)) {
		ngm::pipeline_set_error("out of device memory (ngm_debug_pair_select)"); return -12; }
	MAP_HIP_TRY(hipMemcpy(d_base.p, base, n * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_count.p, count, n * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_len.p, read_len, n * 2, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_mq.p, mapq, n * 4, hipMemcpyHostToDevice));
	MAP_HIP_TRY(hipMemcpy(d_nb.p, n_best, n * 4, hipMemcpyHostToDevice));
	if (n_cand) {
		MAP_HIP_TRY(hipMemcpy(d_sc.p, scores, (size_t) n_cand * 4, hipMemcpyHostToDevice));
		MAP_HIP_TRY(hipMemcpy(d_loc.p, loc, (size_t) n_cand * 4, hipMemcpyHostToDevice));
	}
	// (what no kernel writes reads as -1 everywhere: an entry's `pair` field tells whether it was written)
	MAP_HIP_TRY(hipMemset(d_info.p, 0xFF, (npairs + 1) * 4));
	MAP_HIP_TRY(hipMemset(d_out.p, 0xFF, (2 * npairs + 2) * sizeof(ngm::PairOut)));
	MAP_HIP_TRY(hipMemset(d_top.p, 0xFF, (npairs + 1) * sizeof(ngm::PairTop)));
	MAP_HIP_TRY(hipDeviceSynchronize());
	if (int rc = launch_pair_select(0, npairs, d_base.p, d_count.p, d_sc.p, d_loc.p, d_len.p, min_insert, max_insert, cutoff, d_mq.p, d_nb.p, d_info.p, true,
			d_tied_n.p, d_list.p, d_out.p, d_top.p)) return rc;
	MAP_HIP_TRY(hipDeviceSynchronize());
	MAP_HIP_TRY(hipMemcpy(info, d_info.p, npairs * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(mapq, d_mq.p, n * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(n_best, d_nb.p, n * 4, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(counts, d_tied_n.p, 16, hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(entries, d_out.p, (2 * npairs + 2) * sizeof(ngm::PairOut), hipMemcpyDeviceToHost));
	MAP_HIP_TRY(hipMemcpy(tops, d_top.p, (npairs + 1) * sizeof(ngm::PairTop), hipMemcpyDeviceToHost));
	return 0;
}

int ngm_debug_linear_strings(void *engine, int mode, int n, const char *const *ref, const char *const *qry, const char *dir, uint64_t capacity, void *out_records,
		uint8_t *built_by, uint64_t *cursor) {
	ngm_hip_ctx *ctx = (ngm_hip_ctx *) engine;
	ngm_hip_align_out *out = (ngm_hip_align_out *) out_records;
	if (!ctx || !out || !built_by || !cursor) return -22;
	*cursor = 0;
	if (n <= 0) return 0;
	if (ctx->prm.personality != NGM_PERSONALITY_LINEAR) { ctx->error = "ngm_debug_linear_strings: linear-gap personality only"; return -22; }
	const int am = mode & NGM_MODE_ALIGN_MASK;
	if (am != NGM_MODE_LOCAL && am != NGM_MODE_END_TO_END) { ctx->error = "ngm_debug_linear_strings: unsupported alignment mode"; return -22; }
	DevGuard g(ctx->device);
	auto fail = [&](int rc) { ctx->error = ngm_pipeline_last_error(); return rc; };   // (what the shared launch code reports)
	const size_t rl = ctx->rl, q = ctx->q;
	const int rs = ngm::run_stride(ctx->q, ctx->c);
	const unsigned long long scap = capacity ? capacity : (unsigned long long) n * 96ull + 4096ull;   // 0: the align stage's
	ngm::DevBuf<ngm::CigarDevOut> d_out;
	ngm::DevBuf<char> d_str;
	ngm::DevBuf<uint16_t> d_runs_c;
	ngm::DevBuf<unsigned long long> d_ctr;   // [0] runs, [1] the byte stream's cursor
	if (ctx->h_ref.reserve((size_t) n * rl) || ctx->h_qry.reserve((size_t) n * q) || ctx->d_ref.reserve((size_t) n * rl) || ctx->d_qry.reserve((size_t) n * q) ||
			ctx->d_records.reserve((size_t) n * 8) || ctx->d_runs.reserve((size_t) n * rs) || ctx->h_records.reserve((size_t) n * 8) || d_out.reserve(n) || d_str.reserve(scap) ||
			d_runs_c.reserve((size_t) n * rs) || d_ctr.reserve(2)) { ctx->error = "out of memory (ngm_debug_linear_strings)"; return -12; }
	if (int rc = ngm::engine_stage_dirs(ctx, n, dir)) return rc;
	for (int i = 0; i < n; ++i) {
		memcpy(ctx->h_ref.p + (size_t) i * rl, ref[i], rl);
		memcpy(ctx->h_qry.p + (size_t) i * q, qry[i], q);
	}
	hipStream_t st = ctx->stream;
	if (hipMemcpyAsync(ctx->d_ref.p, ctx->h_ref.p, (size_t) n * rl, hipMemcpyHostToDevice, st) != hipSuccess ||
			hipMemcpyAsync(ctx->d_qry.p, ctx->h_qry.p, (size_t) n * q, hipMemcpyHostToDevice, st) != hipSuccess) { ctx->error = "ngm_debug_linear_strings: upload failed"; return -5; }
	if (int rc = ngm::engine_reserve(ctx, n)) return rc;
	if (int rc = ngm::engine_pack(ctx, n, ctx->d_ref.p, ctx->d_qry.p, st)) return rc;
	const AlignStrings str{d_out.p, d_str.p, scap, d_ctr.p + 1, nullptr, nullptr, ctx->prm.variant, ctx->prm.hard_clip, ctx->prm.silent_clip, ctx->prm.alt_cigar};
	if (int rc = launch_align_strings(ctx, st, mode, n, ctx->d_records.p, ctx->d_runs.p, rs, d_runs_c.p, d_ctr.p, &str, nullptr, nullptr)) return fail(rc);
	std::vector<ngm::CigarDevOut> h_out((size_t) n);
	unsigned long long ctr[2] = {0, 0};
	auto download = [&]() -> int {
		MAP_HIP_TRY(hipMemcpyAsync(h_out.data(), d_out.p, (size_t) n * sizeof(ngm::CigarDevOut), hipMemcpyDeviceToHost, st));
		MAP_HIP_TRY(hipMemcpyAsync(ctr, d_ctr.p, 16, hipMemcpyDeviceToHost, st));
		MAP_HIP_TRY(hipMemcpyAsync(ctx->h_records.p, ctx->d_records.p, (size_t) n * 8 * 4, hipMemcpyDeviceToHost, st));
		MAP_HIP_TRY(hipStreamSynchronize(st));
		return 0;
	};
	if (int rc = download()) return fail(rc);
	if (ctr[0] > (unsigned long long) n * rs) { ctx->error = "ngm_debug_linear_strings: more runs than the scratch holds"; return -75; }
	const unsigned long long used = std::min(ctr[1], scap);
	std::vector<uint16_t> h_runs((size_t) ctr[0] + 1);
	std::vector<char> h_str((size_t) used + 1);
	auto fetch = [&]() -> int {
		if (ctr[0]) MAP_HIP_TRY(hipMemcpy(h_runs.data(), d_runs_c.p, (size_t) ctr[0] * 2, hipMemcpyDeviceToHost));
		if (used) MAP_HIP_TRY(hipMemcpy(h_str.data(), d_str.p, (size_t) used, hipMemcpyDeviceToHost));
		return 0;
	};
	if (int rc = fetch()) return fail(rc);
	*cursor = ctr[1];
	const ngm::CigarParams cp{ctx->prm.match_bonus, -ctx->prm.mismatch_penalty, ctx->prm.variant, ctx->prm.hard_clip, ctx->prm.silent_clip, ctx->prm.alt_cigar};
	for (int i = 0; i < n; ++i) {   // as finish_hits: the device's strings where it built them, the host's builder on the compacted runs otherwise
		const ngm::CigarDevOut &dv = h_out[(size_t) i];
		built_by[i] = (dv.flags & 1) ? 1 : 0;
		if (!(dv.flags & 1)) {
			const int32_t *rec = ctx->h_records.p + (size_t) i * 8;
			if ((uint64_t) (uint32_t) rec[6] + (uint64_t) (rec[0] ? rec[4] : 0) > ctr[0]) { ctx->error = "ngm_debug_linear_strings: runs beyond their total"; return -75; }
			ngm::build_cigar_md(cp, rec, &h_runs[(size_t) (uint32_t) rec[6]], ref[i], qry[i], &out[i], (cp.alt && dir && dir[i]) ? 1 : 0);
			continue;
		}
		if ((unsigned long long) dv.cig_off + dv.cig_len > used || (unsigned long long) dv.md_off + dv.md_len > used) { ctx->error = "ngm_debug_linear_strings: a string beyond the stream"; return -75; }
		memcpy(out[i].cigar, h_str.data() + dv.cig_off, dv.cig_len); out[i].cigar[dv.cig_len] = 0;
		memcpy(out[i].md, h_str.data() + dv.md_off, dv.md_len); out[i].md[dv.md_len] = 0;
		out[i].position_offset = dv.position_offset; out[i].qstart = dv.qstart; out[i].qend = dv.qend;
		out[i].score_token = dv.score_token; out[i].identity = dv.identity; out[i].nm = dv.nm;
	}
	return n;
}

int ngm_debug_gather_pairs(ngm_mapper *m, int n_reads, const char *reads, int n_pairs, const uint32_t *pair_read, const uint32_t *pair_loc, const uint32_t *pair_sv,
		int alt_dir, int align_stage, int dims[2], uint32_t *words, uint16_t *lens, uint16_t *blk_rows) {
	if (!m || !dims) return -22;
	dims[0] = m->eng->RW; dims[1] = m->eng->FW;
	if (!words && !lens && !blk_rows) return 0;   // (the sizes only)
	if (n_reads <= 0 || n_pairs <= 0 || !reads || !pair_read || !pair_loc || !pair_sv || !words || !lens || !blk_rows || alt_dir < 0 || alt_dir > 2) return -22;
	for (int p = 0; p < n_pairs; ++p) if (pair_read[p] >= (uint32_t) n_reads) { ngm::pipeline_set_error("ngm_debug_gather_pairs: pair %d names read %u of %d", p, pair_read[p], n_reads); return -22; }
	DevGuard g(m->ref->device);
	ngm_hip_ctx *eng = m->eng;
	const size_t nb = ((size_t) n_pairs + ngm::kSlots - 1) / ngm::kSlots, n_words = nb * (size_t) (eng->RW + eng->FW) * ngm::kSlots;
	ngm::DevBuf<uint32_t> d_pr, d_pl, d_ps;
	MAP_OOM_TRY(d_pr.reserve(n_pairs) || d_pl.reserve(n_pairs) || d_ps.reserve(n_pairs), "out of device memory (ngm_debug_gather_pairs)");
	if (int rc = ngm::engine_reserve(eng, n_pairs)) { ngm::pipeline_set_error("%s", ngm_hip_last_error(eng)); return rc; }
	// the rows and their lengths as a batch's: uploaded, and searched -- the candidate search measures the reads (its candidates are not used)
	if (int rc = upload_reads(m, n_reads, reads)) return rc;
	m->cs_paired = false;
	if (int rc = run_cs(m, n_reads)) return rc;
	MAP_HIP_TRY(hipMemcpyAsync(d_pr.p, pair_read, (size_t) n_pairs * 4, hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(d_pl.p, pair_loc, (size_t) n_pairs * 4, hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(d_ps.p, pair_sv, (size_t) n_pairs * 4, hipMemcpyHostToDevice, m->st));
	MAP_HIP_TRY(hipMemsetAsync(eng->packed.p, 0xFF, n_words * 4, m->st));   // (a word the kernel leaves out reads as eight classes 15)
	MAP_HIP_TRY(hipMemsetAsync(eng->blk_rows.p, 0xFF, nb * 2, m->st));
	if (int rc = launch_gather(m, window_geom(m, align_stage != 0), d_pr.p, d_pl.p, d_ps.p, n_pairs, alt_dir)) return rc;
	MAP_HIP_TRY(hipMemcpyAsync(words, eng->packed.p, n_words * 4, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(lens, eng->lens.p, (size_t) n_pairs * 2, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipMemcpyAsync(blk_rows, eng->blk_rows.p, nb * 2, hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	return 0;
}

int ngm_mapper_heavy_counters(ngm_mapper *m, uint64_t out[4]) {
	if (!m || !out) return -22;
	out[0] = m->st_heavy_second; out[1] = m->st_heavy_restart; out[2] = m->st_heavy_sent_on; out[3] = m->st_pool_regrown;
	return 0;
}

int ngm_mapper_order_table_reads(ngm_mapper *m, uint64_t *out) {
	if (!m || !out) return -22;
	*out = m->st_order_table;
	return 0;
}

int ngm_mapper_search_turn_counters(ngm_mapper *m, uint64_t out[3]) {
	if (!m || !out) return -22;
	out[0] = m->turn_dbg[0]; out[1] = m->turn_dbg[1]; out[2] = m->turn_dbg[2];
	return 0;
}

int ngm_mapper_cs_dispatch(ngm_mapper *m, uint64_t out[4]) {
	if (!m || !out) return -22;
	out[0] = (uint64_t) m->cs_canon; out[1] = (uint64_t) m->cs_waves; out[2] = (uint64_t) m->last_cs.fast_items; out[3] = (uint64_t) m->last_cs.items16;
	return 0;
}

int ngm_mapper_cs_counters(ngm_mapper *m, uint64_t out[3]) {
	if (!m) return -22;
	out[0] = m->cs_kmers; out[1] = m->cs_hits; out[2] = m->n_cand;
	return 0;
}

float ngm_mapper_last_order_replay_ms(ngm_mapper *m) { return m ? m->order_ms : 0.f; }

int ngm_mapper_last_pair_stats(ngm_mapper *m, uint64_t out[3]) {
	if (!m || !out) return -22;
	out[0] = m->pair_stats[0]; out[1] = m->pair_stats[1]; out[2] = m->pair_stats[2];
	return 0;
}

int ngm_mapper_last_kernel_ms(ngm_mapper *m, float ms[8]) {
	if (!m) return -22;
	for (int i = 0; i < 8; ++i) ms[i] = m->ms[i];
	return 0;
}

}  // extern "C"
