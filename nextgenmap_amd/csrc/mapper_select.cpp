// mapper_select.cpp -- the select stage of a map call (map_impl, mapper.cpp): from behind the score stage's synchronisation to the end of
// the search + score turn.  Host work only -- no kernel is launched here; the candidate order comes from candidate_order
// (mapper_search.cpp), the per-pair logic from pair_host.h:
//   single-end ties (ScoreBuffer::top1SE keeps the first of the best in the reference's candidate order),
//   top1PE for the pairs the GPU has not settled: passes 1-4 around this batch's turn for the running mean insert size (PairSelection),
//   the pairs the reference loses at a full score buffer (reference_buffer_walk), --strata, and -n (ScoreBuffer::topNSE);
// and the two host-only test entries ngm_debug_pair_walk / ngm_debug_pair_eval.
#include "mapper_internal.h"
#include "pair_host.h"

static_assert(ngm::kPairRankUnknown == ngm::kCsOrderUnknown, "pair_host.h and cs_device.h mark an unknown rank alike");

namespace ngm {
namespace {

// several candidates share the read's best score (0: no positive score, the first candidate is kept): the candidate order decides
bool best_is_shared(const MapBatch &b, int i) { return b.h_nbest[i] != 1 && b.m->h_count[i] > 1; }

// ScoreBuffer::top1SE keeps the first of the equally best candidates in ITS candidate order (CollectResultsStd's rList order);
// nothing changes when one of their ranks is unknown
void first_best(MapBatch &b, uint32_t i, const uint32_t *h_rank) {
	ngm_mapper *m = b.m;
	const float *h_scores = b.h_scores;
	const uint32_t base = m->h_base[i], cnt = m->h_count[i];
	if (!h_rank) return;
	float best = h_scores[base];
	for (uint32_t c2 = 1; c2 < cnt; ++c2) best = std::max(best, h_scores[base + c2]);
	uint32_t pick = 0xFFFFFFFFu, pick_rank = ngm::kCsOrderUnknown;
	// (without a positive score top1SE keeps the FIRST candidate, whatever its score: AS:i is that candidate's -- end-to-end mode)
	for (uint32_t c2 = 0; c2 < cnt; ++c2) if (h_scores[base + c2] == best || !(best > 0.0f)) {
		if (h_rank[base + c2] == ngm::kCsOrderUnknown) return;
		if (h_rank[base + c2] < pick_rank) { pick_rank = h_rank[base + c2]; pick = base + c2; }
	}
	if (pick != 0xFFFFFFFFu) { b.h_winner[i] = pick; b.h_best[i] = h_scores[pick]; }
}

// pair_choice_kernel's entries (the pairs with choices only) and the tied pairs' best-scoring combinations
int fetch_pair_choices(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n;
	const size_t npairs = (size_t) n / 2;
	const size_t n_small = std::min<size_t>(m->p_pair_tied_n.p[1], npairs), n_large = std::min<size_t>(m->p_pair_tied_n.p[2], npairs), nt = std::min<size_t>(m->p_pair_tied_n.p[0], npairs);
	MAP_OOM_TRY(m->p_pair_out.reserve(2 * npairs + 2) || m->p_pair_top.reserve(nt + 1), "out of pinned host memory");
	if (n_small) MAP_HIP_TRY(hipMemcpyAsync(m->p_pair_out.p, m->d_pair_out.p, n_small * sizeof(ngm::PairOut), hipMemcpyDeviceToHost, m->st));
	if (n_large) MAP_HIP_TRY(hipMemcpyAsync(m->p_pair_out.p + npairs, m->d_pair_out.p + npairs, n_large * sizeof(ngm::PairOut), hipMemcpyDeviceToHost, m->st));
	if (nt) MAP_HIP_TRY(hipMemcpyAsync(m->p_pair_top.p, m->d_pair_top.p, nt * sizeof(ngm::PairTop), hipMemcpyDeviceToHost, m->st));
	MAP_HIP_TRY(hipStreamSynchronize(m->st));
	return 0;
}

// several candidates share the best score: the reference keeps the first one in ITS candidate order
// (ScoreBuffer::top1SE over CollectResultsStd's rList order); replay the votes of just those reads
int select_single_end_ties(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n;
	const uint64_t np = b.np;
	std::vector<uint32_t> tied;
	for (int i = 0; i < n; ++i) if (best_is_shared(b, i)) tied.push_back((uint32_t) i);
	if (!tied.empty()) {
		uint32_t *h_rank = nullptr;
		if (int rc = candidate_order(m, tied, np, &h_rank)) return rc;
		MAP_OOM_TRY(m->p_scores.reserve(np + 1), "out of pinned host memory");
		b.h_scores = m->p_scores.p;
		MAP_HIP_TRY(hipMemcpy(b.h_scores, m->d_scores.p, np * 4, hipMemcpyDeviceToHost));
		for (uint32_t i : tied) first_best(b, i, h_rank);
	}
	return 0;
}

void reference_buffer_walk(MapBatch &b) {   // inside the batch's turn (sequential state)
	ngm_mapper *m = b.m;
	const int n = b.n;
	std::vector<int> &pair_flags = b.pair_flags;
	uint32_t *h_winner = b.h_winner;
	// A pair the reference LOSES (round 5; the "early top1SE" earlier rounds described does not exist -- MappedRead::Calculated
	// starts at -1, src/MappedRead.cpp:14, so ScoreBuffer.cpp:196 is false while the mate has not been searched).  CS::RunBatch
	// hands a read to its ScoreBuffer right after the search (CS.cpp:436); when the last score of a pair's FIRST mate fills the
	// buffer exactly (ScoreBuffer.cpp:519-523: DoRun), its scores are complete but the mate's Calculated is still -1: nothing is
	// selected.  If the mate then turns out to have NO candidates it goes to the writer alone (CS.cpp:326-329) and no later
	// DoRun ever looks at the first mate again: neither read is written ("(2 discarded)" in the reference's summary;
	// profiles/r05_reference_lost_pair_experiment.txt).  Deterministic at -t 1 for a known buffer size (SeqAn personality:
	// 1 024, src/seqan/EndToEndAffine.h:44-46); mirrored when the caller names that size (ngm_mapper_set_reference_score_buffer).
	// Sequential like the running mean: part of the batch's turn.
	uint64_t tot = m->scores_so_far, at = m->reads_so_far;
	// (the next flush position is carried along: a 64-bit remainder per pair made this loop the longest part of the turn)
	const uint64_t rb = m->ref_cs_batch > 0 ? (uint64_t) m->ref_cs_batch : 0;
	const uint64_t sb = m->ref_score_buffer > 0 ? (uint64_t) m->ref_score_buffer : 0;
	uint64_t next_flush = rb ? (at + rb - 1) / rb * rb : ~0ull;
	uint64_t fill = sb ? tot % sb : 0;   // entries in the reference's score buffer
	for (int pi = 0; pi < n / 2; ++pi, at += 2) {
		while (at > next_flush) next_flush += rb;   // (an odd batch size: flush positions between two pairs never match `at`)
		if (at == next_flush) { tot = 0; fill = 0; next_flush += rb; }  // the reference flushes its score buffer at the end of a CS batch (CS.cpp:488-500)
		const uint32_t c1 = m->h_count[2 * pi], c2 = m->h_count[2 * pi + 1];
		tot += (uint64_t) c1 + c2;
		if (!sb) continue;
		fill += c1;
		const bool full_at_first_mate = c1 > 0 && fill % sb == 0;
		fill = (fill + c2) % sb;
		if (full_at_first_mate && c2 == 0) {
			++m->lost_pairs;
			pair_flags[2 * pi] = pair_flags[2 * pi + 1] = NGM_PAIR_LOST;
			h_winner[2 * pi] = h_winner[2 * pi + 1] = 0xFFFFFFFFu;
		}
	}
	m->scores_so_far = tot; m->reads_so_far = at;
}

// Pairs in input order.  The running mean insert size (tie-break between equally scoring pairs only) is sequential state
// of one CS thread in the reference (pairDistSum / pairDistCount, ScoreBuffer.h:90).  Everything that does not depend on
// it happens outside this batch's turn for that state -- on the GPU (pair_simple_kernel, pair_choice_kernel) or in
// parallel on the host -- and the turn itself only scans what is left (NGM_HIP_HOST_THREADS=1: strictly sequential).
struct PairSelection {
	MapBatch &b;
	ngm_mapper *const m;
	const int n, q;
	const char *const reads;
	const uint64_t np;
	uint32_t *const h_winner, *const h_loc, *const h_sv;
	int32_t *const h_mapq, *const h_nbest;
	float *const h_best, *const h_scores;
	std::vector<int> &pair_flags;
	PairTurn &pair_turn;
	const bool simple_on_gpu, choice_on_gpu;
	const bool pe_strata;
	// Pass 1: every pair whose result depends on the scores alone -- nearly all of them -- is settled.  The others ("tied":
	// equally scoring pairs inside the window) depend on the running mean insert size, and some also on the candidate order.
	// gap_*: insert sizes / number of the pairs selected since the previous tied pair; dist: this pair's once it is closed;
	// seq: its in-window combinations in the reference's order (pass 3), or -1
	struct Tied { int pi; bool found, dup, open; int dmin, dmax, mqa, mqb; long avg_lo, avg_hi; int n_top, top_d[8], top_a[8], top_b[8]; long gap_sum, gap_cnt; int dist; int seq; };
	struct Chunk { int plo; std::vector<Tied> tied; std::vector<uint32_t> se; long tail_sum, tail_cnt; };
	static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
	std::chrono::steady_clock::time_point tq0 = now(); double tq[5] = {0, 0, 0, 0, 0};
	void qlap(int k) { auto t = now(); tq[k] += std::chrono::duration<double, std::milli>(t - tq0).count(); tq0 = t; }
	std::mutex tied_mu;
	std::vector<Tied> tied;
	std::vector<uint32_t> se_tied;  // mates selected single-end (no pair in the window / mate without candidates) whose best score is shared
	std::vector<Chunk> chunks;
	std::atomic<long> n_host_walk{0};
	long carry_sum = 0, carry_cnt = 0;  // selected pairs after the last tied pair so far
	std::vector<int> picked;   // indices into `tied`
	std::vector<int> late;   // left open without having been picked above
	std::vector<PairSeq> seqs;
	uint32_t *h_rank_pe = nullptr;
	size_t n_open = 0;

	explicit PairSelection(MapBatch &b_) : b(b_), m(b_.m), n(b_.n), q(b_.q), reads(b_.reads), np(b_.np), h_winner(b_.h_winner), h_loc(b_.h_loc), h_sv(b_.h_sv),
		h_mapq(b_.h_mapq), h_nbest(b_.h_nbest), h_best(b_.h_best), h_scores(b_.h_scores), pair_flags(b_.pair_flags), pair_turn(b_.pair_turn),
		simple_on_gpu(b_.simple_on_gpu), choice_on_gpu(b_.choice_on_gpu), pe_strata(b_.m->prm.strata != 0) {}

	void commit(int ra, int rb, bool found, int wa, int wb, int mqa, int mqb, int equal) {
		if (found && pe_strata && equal > 0) {  // "To many equal scoring positions": both mates unmapped (ScoreBuffer.cpp:437-446)
			h_winner[ra] = h_winner[rb] = 0xFFFFFFFFu;
			h_mapq[ra] = h_mapq[rb] = 0;
			pair_flags[ra] = pair_flags[rb] = NGM_PAIR_SELECTED;
		} else if (found) {
			h_winner[ra] = (uint32_t) wa; h_winner[rb] = (uint32_t) wb;
			h_mapq[ra] = mqa; h_mapq[rb] = mqb;
			h_nbest[ra] = h_nbest[rb] = equal;
			h_best[ra] = h_scores[wa]; h_best[rb] = h_scores[wb];
			pair_flags[ra] = pair_flags[rb] = NGM_PAIR_SELECTED;
		} else {
			pair_flags[ra] = pair_flags[rb] = NGM_PAIR_FAILED;  // no pair inside the window: single-end selection stands
		}
	}
	int len_of(int rd) const { return (int) strnlen(reads + (size_t) rd * q, q); }
	void run_pair(int pi, long sum, long cnt, const uint32_t *rank, int *wa, int *wb, int *mqa, int *mqb, int *equal, int *dist, bool *found, PairTies *ties) {
		const int rb = 2 * pi, ra = 2 * pi + 1;
		select_pair(m->prm, sum, cnt, dist, m->h_base[ra], m->h_count[ra], len_of(ra), m->h_base[rb], m->h_count[rb], len_of(rb), h_loc, h_sv, h_scores, rank, wa, wb, mqa, mqb, equal, found, ties);
	}
	void se_check(std::vector<uint32_t> &out, int i) { if (best_is_shared(b, i)) out.push_back((uint32_t) i); }

	void pass1() {
		const ngm::PairOut *h_po = choice_on_gpu ? m->p_pair_out.p : nullptr;
		const ngm::PairTop *h_pt = choice_on_gpu ? m->p_pair_top.p : nullptr;
		parallel_for(n / 2, [&](int plo, int phi) {
			// (what the loop reads at every pair, as locals of the chunk)
			ngm_mapper *const m = this->m;
			const int n = this->n;
			const bool simple_on_gpu = this->simple_on_gpu;
			int *const pair_flags = this->pair_flags.data();
			std::vector<Tied> local;
			std::vector<uint32_t> local_se;
			long gsum = 0, gcnt = 0, walked = 0;
			for (int pi = plo; pi < phi; ++pi) {
				const int rb = 2 * pi, ra = 2 * pi + 1;
				const int pinfo = simple_on_gpu ? m->p_pair_info.p[pi] : -1;
				if (simple_on_gpu && pinfo >= 0) {   // one candidate per mate: pair_simple_kernel has settled it
					const int info = m->p_pair_info.p[pi];
					if (info & 1) { pair_flags[ra] = pair_flags[rb] = NGM_PAIR_SELECTED; gsum += info >> 1; ++gcnt; }
					else pair_flags[ra] = pair_flags[rb] = NGM_PAIR_FAILED;
					continue;
				}
				if (m->h_count[ra] == 0 || m->h_count[rb] == 0) { se_check(local_se, rb); se_check(local_se, ra); continue; }  // top1SE for the mate that has candidates (ScoreBuffer.cpp:204-209)
				const ngm::PairOut *pe = nullptr;
				if (h_po && pinfo <= -2) { const uint32_t e = (uint32_t) (-2 - (long long) pinfo); pe = &h_po[e >= (1u << 30) ? (size_t) (n / 2) + (e - (1u << 30)) : e]; }
				if (pe && !(pe->flags & ngm::kPairHost)) {   // pair_choice_kernel: settled, or what the sequential passes need
					const ngm::PairOut &po = *pe;
					const bool found = (po.flags & ngm::kPairFound) != 0;
					const int mqa = (po.flags >> 8) & 255, mqb = (po.flags >> 16) & 255;
					if (po.flags & ngm::kPairTied) {
						Tied t{pi, found, (po.flags & ngm::kPairDup) != 0, true, po.dmin, po.dmax, mqa, mqb, 0, 0, std::min((po.flags >> 24) & 15, 8), {}, {}, {}, gsum, gcnt, 0, -1};
						gsum = gcnt = 0;
						const ngm::PairTop &pt = h_pt[po.tied_ix];
						for (int x = 0; x < t.n_top; ++x) { t.top_d[x] = pt.d[x]; t.top_a[x] = pt.a[x]; t.top_b[x] = pt.b[x]; }
						local.push_back(t);
						continue;
					}
					commit(ra, rb, found, po.wa, po.wb, mqa, mqb, 0);
					if (found) { gsum += po.dist; ++gcnt; } else { se_check(local_se, rb); se_check(local_se, ra); }
					continue;
				}
				++walked;
				int wa = -1, wb = -1, mqa = 0, mqb = 0, equal = 0, dist = 0;
				bool found = false;
				PairTies ties;
				run_pair(pi, 0, 1, nullptr, &wa, &wb, &mqa, &mqb, &equal, &dist, &found, &ties);
				if (ties.equal_scores) {
					Tied t{pi, found, ties.dup || pe_strata, true, ties.dmin_top, ties.dmax_top, mqa, mqb, 0, 0, std::min(ties.n_top, 8), {}, {}, {}, gsum, gcnt, 0, -1};
					gsum = gcnt = 0;
					for (int x = 0; x < t.n_top; ++x) { t.top_d[x] = ties.top_d[x]; t.top_a[x] = ties.top_a[x]; t.top_b[x] = ties.top_b[x]; }
					local.push_back(t);
					continue;
				}
				commit(ra, rb, found, wa, wb, mqa, mqb, equal);
				if (found) { gsum += dist; ++gcnt; } else { se_check(local_se, rb); se_check(local_se, ra); }
			}
			n_host_walk += walked;
			{ std::lock_guard<std::mutex> lk(tied_mu); chunks.push_back(Chunk{plo, std::move(local), std::move(local_se), gsum, gcnt}); }
		});
		std::sort(chunks.begin(), chunks.end(), [](const Chunk &x, const Chunk &y) { return x.plo < y.plo; });  // pairs in input order again
		for (Chunk &c : chunks) {
			if (!c.tied.empty()) { c.tied[0].gap_sum += carry_sum; c.tied[0].gap_cnt += carry_cnt; carry_sum = carry_cnt = 0; }
			carry_sum += c.tail_sum; carry_cnt += c.tail_cnt;
			tied.insert(tied.end(), c.tied.begin(), c.tied.end());
			se_tied.insert(se_tied.end(), c.se.begin(), c.se.end());
		}
		// a tied pair without a positive pair score fails whatever the mean: single-end selection for both mates
		for (Tied &t : tied) if (!t.found) {
			commit(2 * t.pi + 1, 2 * t.pi, false, -1, -1, 0, 0, 0);
			se_check(se_tied, 2 * t.pi); se_check(se_tied, 2 * t.pi + 1);
			t.open = false;
		}
	}

	// Which tied pairs will stay open in the sequential pass?  Those whose equally scoring pairs also share the insert size
	// (`dup`: the candidate order decides) -- and those whose best-scoring pair closest to the mean is not the same unique one
	// over the range the mean can have when their turn comes.  That range is only known inside the turn (pass 2 carries exact
	// bounds); the mean of thousands of insert sizes hardly moves, so outside the turn pass 2 runs SPECULATIVELY from the last
	// PUBLISHED mean +- 3 -- bounds that contain the exact ones leave a superset of the exact pass's pairs open -- and the pairs
	// it leaves open have their candidate order replayed and their combinations listed (pass 3) before the turn begins.  A
	// pair that the exact pass 2 leaves open without having been picked here (the first batches of a run, while the mean still
	// moves by more than 3) is handled inside the turn, as every open pair was before round 5.
	static int closest_top(const Tied &t, long avg, bool *unique) {
		int best = 0, n_best = 0; long best_c = LONG_MAX;
		for (int x = 0; x < t.n_top; ++x) {
			const long cx = labs((long) t.top_d[x] - avg);
			if (cx < best_c) { best_c = cx; best = x; n_best = 1; } else if (cx == best_c) ++n_best;
		}
		*unique = n_best == 1;
		return best;
	}
	static bool closed_between(const Tied &t, long lo, long hi, int *which) {
		if (t.dup || t.n_top <= 0) return false;
		bool u_lo = false, u_hi = false;
		const int x_lo = closest_top(t, lo, &u_lo), x_hi = closest_top(t, hi, &u_hi);
		*which = x_lo;
		return x_lo == x_hi && u_lo && u_hi;
	}
	// pass 2 itself (see below), from a given state of the running mean: exact -- it commits what it closes -- or speculative
	void pass2(long sum_lo, long sum_hi, long cnt, bool exact, std::vector<int> &left_open) {
		for (size_t x = 0; x < tied.size(); ++x) {
			Tied &t = tied[x];
			sum_lo += t.gap_sum; sum_hi += t.gap_sum; cnt += t.gap_cnt;
			const long a_lo = sum_lo / std::max(1L, cnt), a_hi = sum_hi / std::max(1L, cnt);
			if (exact) { t.avg_lo = a_lo; t.avg_hi = a_hi; }
			if (!t.found) continue;
			int which = 0;
			if (closed_between(t, a_lo, a_hi, &which)) {
				if (exact) {
					commit(2 * t.pi + 1, 2 * t.pi, true, t.top_a[which], t.top_b[which], t.mqa, t.mqb, 0);
					t.dist = t.top_d[which];
					t.open = false;
				}
				sum_lo += t.top_d[which]; sum_hi += t.top_d[which]; ++cnt;
				continue;
			}
			left_open.push_back((int) x);
			sum_lo += t.dmin; sum_hi += t.dmax; ++cnt;
		}
	}
	void build_seq(PairSeq &sq, int pi) {
		const int rb = 2 * pi, ra = 2 * pi + 1;
		// (only the combinations that reach the running maximum of the pair score are kept: eval_pair_seq does nothing at the others
		// whatever the mean -- its `top` is the maximum so far, starting at 0 -- and a pair of two satellite-array mates has
		// hundreds of thousands of them)
		walk_pair(m->prm, m->h_base[ra], m->h_count[ra], len_of(ra), m->h_base[rb], m->h_count[rb], len_of(rb), h_loc, h_sv, h_scores, h_rank_pe, &sq.mq_a, &sq.mq_b,
				PairSeqKeeper{sq});
	}
	// ... but when both mates have candidates top1PE has already SORTED the arrays before it falls back to
	// top1SE (ScoreBuffer.cpp:373-376, 449-455): the first of the best is the head of that (unstable) sort
	void first_sorted(uint32_t i) {
		if (!h_rank_pe) return;
		// (also for the <= 16 candidates of a stable insertion sort: the head of the sorted array is the BEST score's first candidate --
		// without a positive score top1SE then keeps it, not the first candidate of the unsorted list: end-to-end mode)
		bool ranked = false;
		std::vector<uint32_t> v(m->h_count[i]);
		sort_like_reference(v.data(), m->h_base[i], m->h_count[i], h_loc, h_sv, h_scores, h_rank_pe, &ranked);
		if (ranked) { h_winner[i] = v[0]; h_best[i] = h_scores[v[0]]; }
	}

	// outside the turn: the speculative pass 2, the order replay of what it leaves open and of the single-end ties, pass 3
	int before_turn() {
		long pub_sum = m->pair_dist_sum, pub_cnt = m->pair_dist_count;
		if (m->ps && !pair_turn.held) { std::lock_guard<std::mutex> lk(m->ps->mu); pub_sum = m->ps->dist_sum; pub_cnt = m->ps->dist_count; }
		if (pe_strata) { for (size_t x = 0; x < tied.size(); ++x) if (tied[x].found) picked.push_back((int) x); }
		else pass2(pub_sum - 3 * pub_cnt, pub_sum + 3 * pub_cnt, pub_cnt, false, picked);   // (bounds that contain the exact ones leave a superset of the exact pass's pairs open)
		std::vector<uint32_t> need;
		need.reserve(2 * picked.size() + se_tied.size());
		for (int x : picked) { need.push_back((uint32_t) (2 * tied[x].pi)); need.push_back((uint32_t) (2 * tied[x].pi + 1)); }
		need.insert(need.end(), se_tied.begin(), se_tied.end());
		qlap(0);
		if (!need.empty()) if (int rc = candidate_order(m, need, np, &h_rank_pe)) return rc;
		qlap(1);
		// Pass 3 (parallel, outside the turn): the in-window combinations of the picked pairs in the reference's order
		seqs.resize(picked.size());
		parallel_for((int) picked.size(), [&](int lo, int hi) { for (int x = lo; x < hi; ++x) { build_seq(seqs[x], tied[picked[x]].pi); tied[picked[x]].seq = x; } }, 8);
		qlap(2);
		// the single-end ties do not touch the mean: settled here, in parallel
		parallel_for((int) se_tied.size(), [&](int lo, int hi) { for (int x = lo; x < hi; ++x) { const uint32_t i = se_tied[x]; if (m->h_count[i ^ 1u] > 0) first_sorted(i); else first_best(b, i, h_rank_pe); } }, 64);
		return 0;
	}

	// ---- this batch's turn for the running mean ----------------------------------------------------------------------
	int turn() {
		pair_turn.acquire();
		reference_buffer_walk(b);
		// Pass 2 (sequential, cheap): the running mean at every tied pair, as bounds -- a tied pair that stays open contributes one
		// of the insert sizes of its best-scoring pairs.  Without pairs of equal score AND insert size the winner is the
		// best-scoring pair closest to the mean: the same unique winner at both bounds is the winner for every mean in between,
		// and its insert size keeps the bounds exact.  (With --strata a tied pair may contribute nothing at all; then every tied
		// pair simply waits for pass 4.)
		if (!pe_strata) {
			std::vector<int> left_open;
			pass2(m->pair_dist_sum, m->pair_dist_sum, m->pair_dist_count, true, left_open);
			for (int x : left_open) if (tied[x].seq < 0) late.push_back(x);
		}
		qlap(3);
		for (const Tied &t : tied) n_open += t.open;
		if (!late.empty()) {
			std::vector<uint32_t> need_late;
			for (int x : late) { need_late.push_back((uint32_t) (2 * tied[x].pi)); need_late.push_back((uint32_t) (2 * tied[x].pi + 1)); }
			if (int rc = candidate_order(m, need_late, np, &h_rank_pe)) return rc;
			const size_t s0 = seqs.size();
			seqs.resize(s0 + late.size());
			parallel_for((int) late.size(), [&](int lo, int hi) { for (int x = lo; x < hi; ++x) { build_seq(seqs[s0 + x], tied[late[x]].pi); tied[late[x]].seq = (int) (s0 + x); } }, 8);
		}
		// Pass 4 (sequential): the running mean in input order; the open pairs see exactly the reference's value
		for (const Tied &t : tied) {
			const int pi = t.pi;
			m->pair_dist_sum += t.gap_sum; m->pair_dist_count += t.gap_cnt;
			if (!t.open) { if (t.dist) { m->pair_dist_sum += t.dist; m->pair_dist_count += 1; } continue; }  // closed by pass 2 (or not found)
			const PairOutcome o = eval_pair_seq(seqs[t.seq], (int) (m->pair_dist_sum / std::max(1L, m->pair_dist_count)));
			const int rb = 2 * pi, ra = 2 * pi + 1;
			commit(ra, rb, o.found, o.wa, o.wb, o.mqa, o.mqb, o.equal);
			if (o.found && !(pe_strata && o.equal > 0)) { m->pair_dist_sum += o.dist; m->pair_dist_count += 1; }
			if (!o.found) { if (best_is_shared(b, ra)) first_sorted((uint32_t) ra); if (best_is_shared(b, rb)) first_sorted((uint32_t) rb); }
		}
		m->pair_dist_sum += carry_sum; m->pair_dist_count += carry_cnt;
		pair_turn.release();
		qlap(4);
		return 0;
	}

	void report() const {   // NGM_HIP_HOST_TIMING
		g_walk_probe = true;
		const double pn = (double) std::max<uint64_t>(1, g_walk_ns[5].load());
		fprintf(stderr, "[ngm-hip] pair walks so far: %.0f pairs; per pair: sorts %.1f us, rest of the walk %.1f us, %.0f candidates, %.0f above the cut-off, %.0f combinations looked at\n", pn,
				g_walk_ns[0].load() / pn / 1e3, g_walk_ns[1].load() / pn / 1e3, g_walk_ns[2].load() / pn, g_walk_ns[3].load() / pn, g_walk_ns[4].load() / pn);
		fprintf(stderr, "[ngm-hip] pair selection: %zu tied pairs, %zu picked for the order replay + %zu single-end ties, %zu open in the turn, %zu of them late; %ld pairs walked on the host; "
				"ms: pass 1 %.2f | order replay %.2f | pass 3 %.2f | turn: pass 2 %.2f, late + pass 4 %.2f\n", tied.size(), picked.size(), se_tied.size(), n_open, late.size(), (long) n_host_walk, tq[0], tq[1], tq[2], tq[3], tq[4]);
	}
};

// ScoreBuffer::topNSE: sort by score, report min(topn, candidates) (strata: the equally best ones only)
int select_topn(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n, topn = b.topn;
	const uint64_t np = b.np;
	uint32_t *h_winner = b.h_winner, *h_loc = b.h_loc, *h_sv = b.h_sv;
	int32_t *h_mapq = b.h_mapq, *h_nbest = b.h_nbest;
	float *h_best = b.h_best;
	std::vector<uint32_t> &tn_pairs = b.tn_pairs;
	MAP_OOM_TRY(m->p_scores.reserve(np + 1), "out of pinned host memory");
	float *h_scores = b.h_scores = m->p_scores.p;
	MAP_HIP_TRY(hipMemcpy(h_scores, m->d_scores.p, np * 4, hipMemcpyDeviceToHost));
	tn_pairs.assign((size_t) n * topn, 0xFFFFFFFFu);
	// equally scoring candidates keep the reference's candidate order (the cut at -n is order dependent)
	uint32_t *h_rank_tn = nullptr;
	{
		std::vector<uint32_t> need;
		for (int i = 0; i < n; ++i) {
			const uint32_t b = m->h_base[i], cnt = m->h_count[i];
			bool eq = false;
			for (uint32_t x = 0; x + 1 < cnt && !eq; ++x) for (uint32_t y = x + 1; y < cnt; ++y) if (h_scores[b + x] == h_scores[b + y]) { eq = true; break; }
			if (eq) need.push_back((uint32_t) i);
		}
		if (!need.empty()) if (int rc = candidate_order(m, need, np, &h_rank_tn)) return rc;
	}
	parallel_for(n, [&](int lo, int hi) {
		std::vector<uint32_t> v;
		for (int i = lo; i < hi; ++i) {
			const uint32_t b = m->h_base[i], cnt = m->h_count[i];
			if (cnt == 0) continue;
			v.resize(cnt);
			std::iota(v.begin(), v.end(), b);
			// std::sort(sortLocationScore) over the reference's candidate order, as in select_pair
			auto by_place = [&](uint32_t x, uint32_t y) { return h_loc[x] != h_loc[y] ? h_loc[x] < h_loc[y] : (h_sv[x] & 1u) < (h_sv[y] & 1u); };
			bool ranked = h_rank_tn != nullptr;
			for (uint32_t x = b; ranked && x < b + cnt; ++x) ranked = h_rank_tn[x] != ngm::kCsOrderUnknown;
			if (ranked) {
				std::sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return h_rank_tn[x] != h_rank_tn[y] ? h_rank_tn[x] < h_rank_tn[y] : by_place(x, y); });
				std::sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return h_scores[x] > h_scores[y]; });
			} else {
				std::sort(v.begin(), v.end(), by_place);
				std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return h_scores[x] > h_scores[y]; });
			}
			int ntop = 1;
			while (ntop < (int) cnt && h_scores[v[0]] == h_scores[v[ntop]]) ++ntop;
			h_nbest[i] = ntop;
			int ns = 0;
			if (ntop <= topn || !m->prm.strata) {
				ns = m->prm.strata ? ntop : std::min<int>((int) cnt, topn);
				int mq = 60;  // computeMQ(MappedRead*)
				if (cnt > 1) { const float bs = h_scores[v[0]], s2 = h_scores[v[1]]; mq = (bs > 0 && s2 >= 0) ? (int) ceilf(60.0f * (bs - s2) / bs) : 0; }
				h_mapq[i] = mq;
			} else {
				h_mapq[i] = 0;
			}
			for (int t = 0; t < ns; ++t) tn_pairs[(size_t) i * topn + t] = v[t];
			h_winner[i] = ns > 0 ? v[0] : 0xFFFFFFFFu;
			h_best[i] = h_scores[v[0]];
		}
	});
	return 0;
}

}  // namespace

int select(MapBatch &b) {
	ngm_mapper *m = b.m;
	const int n = b.n;
	const bool paired = b.paired;
	const uint64_t np = b.np;
	uint32_t *h_winner = b.h_winner;
	int32_t *h_mapq = b.h_mapq, *h_nbest = b.h_nbest;
	std::vector<int> &pair_flags = b.pair_flags;
	if (np > 0) {
		if (int rc = cs_host_arrays(m)) return rc;
		if (b.choice_on_gpu) if (int rc = fetch_pair_choices(b)) return rc;
		b.lap(1);
		if ((!paired || m->fast_pairing) && m->prm.topn <= 1) if (int rc = select_single_end_ties(b)) return rc;
		if (b.pe_select) {
			PairSelection ps(b);
			ps.pass1();
			if (int rc = ps.before_turn()) return rc;
			if (int rc = ps.turn()) return rc;
			if (b.host_timing) ps.report();
		}
	}
	if (paired && (np == 0 || m->fast_pairing)) { b.pair_turn.acquire(); reference_buffer_walk(b); b.pair_turn.release(); }   // (--fast-pairing / a batch without candidates: no top1PE turn above)
	if (paired && np > 0 && m->prm.strata)  // mates selected single-end (top1SE): several equally best candidates -> unmapped
		parallel_for(n, [&](int lo, int hi) { for (int i = lo; i < hi; ++i) if (!(pair_flags[i] & NGM_PAIR_SELECTED) && h_nbest[i] > 1) { h_winner[i] = 0xFFFFFFFFu; h_mapq[i] = 0; } }, 16384);
	const int topn = b.topn = (!paired && m->prm.topn > 1) ? m->prm.topn : 1;
	if (!paired && np > 0 && (topn > 1 || m->prm.strata)) {
		if (topn == 1) {  // top1SE with strata: several equally best candidates -> unmapped (ScoreBuffer.cpp:259-276)
			for (int i = 0; i < n; ++i) if (h_nbest[i] > 1) { h_winner[i] = 0xFFFFFFFFu; h_mapq[i] = 0; }
		} else if (int rc = select_topn(b)) return rc;
	}
	b.stage_cs.done();
	b.lap(2);
	return 0;
}

}  // namespace ngm

extern "C" {

// Debug / test entry, host only (no GPU): the part of top1PE that pass 3 of the pair selection runs per tied pair -- both candidate lists
// sorted as the reference sorts them (candidate order from `rank`, then std::sort by score), the MAPQs, and the in-window combinations of
// the candidates above the cut-off in the order of the reference's double loop.  out_a / out_b: the sorted lists (indices into loc / sv /
// score / rank; cnt_a and cnt_b entries); combo_*: at most `cap` combinations, *n_combo their number (all of them counted).
// tests/test_pair_walk.py compares it with a restatement of libstdc++'s std::sort and the plain double loop.
int ngm_debug_pair_walk(uint32_t cnt_a, int len_a, uint32_t cnt_b, int len_b, const uint32_t *loc, const uint32_t *sv, const float *score, const uint32_t *rank,
		float cutoff, int min_insert, int max_insert, uint32_t *out_a, uint32_t *out_b, int *mq_a, int *mq_b, uint64_t cap, float *combo_score, int *combo_dist, int *combo_a, int *combo_b,
		uint64_t *n_combo) {
	if (!cnt_a || !cnt_b || !loc || !sv || !score || !out_a || !out_b || !mq_a || !mq_b || !n_combo) { ngm::pipeline_set_error("ngm_debug_pair_walk: bad arguments"); return -1; }
	ngm_mapper_params prm{};
	prm.pair_score_cutoff = cutoff; prm.min_insert_size = min_insert; prm.max_insert_size = max_insert;
	sort_like_reference(out_a, 0, cnt_a, loc, sv, score, rank);
	sort_like_reference(out_b, cnt_a, cnt_b, loc, sv, score, rank);
	uint64_t n = 0;
	walk_pair(prm, 0, cnt_a, len_a, cnt_a, cnt_b, len_b, loc, sv, score, rank, mq_a, mq_b, [&](float ps, int cur, int ia, int ib) {
		if (n < cap && combo_score && combo_dist && combo_a && combo_b) { combo_score[n] = ps; combo_dist[n] = cur; combo_a[n] = ia; combo_b[n] = ib; }
		++n;
	});
	*n_combo = n;
	return 0;
}

// Debug / test entry, host only: the double loop of top1PE over CheckPairs at running mean `avg` (eval_pair_seq) on a given sequence of
// in-window combinations -- once on all of them, once on what PairSeqKeeper keeps.  out[6]: found, winner of a, winner of b, pairs of
// equal score and insert size, insert size, combinations evaluated.
int ngm_debug_pair_eval(uint64_t n, const float *pair_score, const int *dist, const int *ia, const int *ib, int avg, int out_all[6], int out_kept[6]) {
	if ((n && (!pair_score || !dist || !ia || !ib)) || !out_all || !out_kept) { ngm::pipeline_set_error("ngm_debug_pair_eval: bad arguments"); return -1; }
	PairSeq all, kept;
	PairSeqKeeper keep{kept};
	for (uint64_t x = 0; x < n; ++x) {
		all.ps.push_back(pair_score[x]); all.d.push_back(dist[x]); all.a.push_back(ia[x]); all.b.push_back(ib[x]);
		keep(pair_score[x], dist[x], ia[x], ib[x]);
	}
	auto put = [](const PairSeq &q, int avg_, int *o) {
		const PairOutcome r = eval_pair_seq(q, avg_);
		o[0] = r.found ? 1 : 0; o[1] = r.wa; o[2] = r.wb; o[3] = r.equal; o[4] = r.dist; o[5] = (int) q.ps.size();
	};
	put(all, avg, out_all); put(kept, avg, out_kept);
	return 0;
}

}  // extern "C"
