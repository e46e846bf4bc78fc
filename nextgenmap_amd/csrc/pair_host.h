// pair_host.h -- the host's part of the paired-end selection that is pure logic (no GPU, no mapper state): ScoreBuffer::top1PE and
// CheckPairs (src/ScoreBuffer.cpp:368-502) on one pair's candidate arrays.  The reference's two sorts (sort_like_reference), the walk over
// the in-window combinations in the order of its double loop (walk_pair), the scan over kept combinations at a given running mean
// (PairSeq, PairSeqKeeper, eval_pair_seq) and the whole selection of one pair with what it learns about ties (select_pair, PairTies).
// mapper_select.cpp runs them per pair; tests/cpp/pair_host_driver.cpp builds them with plain g++ (tests/test_pair_host.py).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../include/ngm_pipeline.h"

namespace ngm {
constexpr uint32_t kPairRankUnknown = 0xFFFFFFFFu;   // a candidate whose place in the reference's order is not known (= kCsOrderUnknown, cs_device.h)
}

// ScoreBuffer::top1PE's std::sort(Scores, sortLocationScore) (src/ScoreBuffer.cpp:373-376) over one read's candidates.
static void sort_like_reference(uint32_t *v, uint32_t base, uint32_t cnt, const uint32_t *loc, const uint32_t *sv, const float *score, const uint32_t *rank,
	bool *ranked_out = nullptr) {
	std::iota(v, v + cnt, base);
	// The reference sorts its candidate list (CollectResultsStd's order) with std::sort(sortLocationScore): an insertion
	// sort -- stable -- up to 16 elements, an unstable introsort above, so there do exactly that on the same sequence.
	// Without the candidate order (first pass; only pairs whose result does not depend on it are kept) any deterministic
	// order will do.
	auto by_place = [&](uint32_t x, uint32_t y) { return loc[x] != loc[y] ? loc[x] < loc[y] : (sv[x] & 1u) < (sv[y] & 1u); };
	bool ranked = rank != nullptr;
	for (uint32_t x = base; ranked && x < base + cnt; ++x) ranked = rank[x] != ngm::kPairRankUnknown;
	if (ranked_out) *ranked_out = ranked;
	if (!ranked) {
		if (cnt > 64) {   // (a total order: any algorithm gives the same result -- sorted as records, not through the index arrays)
			struct Rec { float s; uint32_t l, st, i; };
			thread_local std::vector<Rec> recs;
			recs.resize(cnt);
			for (uint32_t x = 0; x < cnt; ++x) { const uint32_t i = base + x; recs[x] = Rec{score[i], loc[i], sv[i] & 1u, i}; }
			std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.s != b.s ? a.s > b.s : a.l != b.l ? a.l < b.l : a.st < b.st; });
			for (uint32_t x = 0; x < cnt; ++x) v[x] = recs[x].i;
			return;
		}
		std::sort(v, v + cnt, [&](uint32_t x, uint32_t y) { return score[x] != score[y] ? score[x] > score[y] : by_place(x, y); });
		return;
	}
	auto by_rank = [&](uint32_t x, uint32_t y) { return rank[x] != rank[y] ? rank[x] < rank[y] : by_place(x, y); };
	if (cnt <= 16) { std::sort(v, v + cnt, [&](uint32_t x, uint32_t y) { return score[x] != score[y] ? score[x] > score[y] : by_rank(x, y); }); return; }
	// Round 6: the same two sorts on VALUES instead of through the index arrays (a read of a repeat family has thousands of candidates, and
	// the stress sub-leg of the bench sorts ~10 000 such lists per batch on a 16-CPU quota: every comparison was two or four cache misses).
	// (1) the reference's candidate order: ranks are distinct (2 x the entering time of the bin + strand), so (rank << 32 | index) sorts as
	// integers -- should two ranks ever be equal, the comparator path below decides as before; (2) std::sort by score on (score, index)
	// records in that order: the same algorithm asked the same questions in the same sequence moves the same elements.
	{
		thread_local std::vector<uint64_t> keys;
		struct Rec { float s; uint32_t i; };
		thread_local std::vector<Rec> recs;
		keys.resize(cnt);
		uint32_t rank_or = 0;
		for (uint32_t x = 0; x < cnt; ++x) { keys[x] = ((uint64_t) rank[base + x] << 32) | (uint64_t) (base + x); rank_or |= rank[base + x]; }
		if (cnt < 256) std::sort(keys.begin(), keys.end());
		else {
			// ranks are 2 x a hit time + strand: 21-23 bits -- two or three stable passes of 11 bits (equal ranks, should there be any, keep the
			// index order they were written in: what the integer sort of (rank, index) gives)
			thread_local std::vector<uint64_t> tmp;
			tmp.resize(cnt);
			uint64_t *src = keys.data(), *dst = tmp.data();
			for (int sh = 32; sh < 64 && (rank_or >> (sh - 32)) != 0u; sh += 11) {
				uint32_t hist[2048] = {0};
				for (uint32_t x = 0; x < cnt; ++x) ++hist[(src[x] >> sh) & 2047u];
				uint32_t run = 0;
				for (uint32_t h = 0; h < 2048; ++h) { const uint32_t c = hist[h]; hist[h] = run; run += c; }
				for (uint32_t x = 0; x < cnt; ++x) dst[hist[(src[x] >> sh) & 2047u]++] = src[x];
				std::swap(src, dst);
			}
			if (src != keys.data()) std::copy(src, src + cnt, keys.data());
		}
		bool distinct = true;
		for (uint32_t x = 1; x < cnt && distinct; ++x) distinct = (keys[x] >> 32) != (keys[x - 1] >> 32);
		if (distinct) {
			recs.resize(cnt);
			for (uint32_t x = 0; x < cnt; ++x) { const uint32_t i = (uint32_t) keys[x]; recs[x] = Rec{score[i], i}; }
			std::sort(recs.begin(), recs.end(), [](const Rec &a, const Rec &b) { return a.s > b.s; });
			for (uint32_t x = 0; x < cnt; ++x) v[x] = recs[x].i;
			return;
		}
	}
	std::sort(v, v + cnt, by_rank);
	std::sort(v, v + cnt, [&](uint32_t x, uint32_t y) { return score[x] > score[y]; });
}

// What select_pair learns about the equally scoring pairs of one read pair (see the comment at the end of select_pair).
struct PairTies {
	PairTies() {}  // the arrays stay uninitialised: this is constructed once per pair
	bool equal_scores = false;   // two in-window pairs share a pair score: the running mean insert size is consulted
	bool dup = false;            // ... and two of them also share the insert size: the candidate order decides, NH/X0 counts them
	bool unique_closest = true;  // at the mean passed in, exactly one best-scoring pair is closest to it
	int dmin_top = 0, dmax_top = 0;  // range of the insert sizes of the best-scoring pairs
	int n_top = 0;               // the best-scoring pairs themselves (insert size, candidates), at most 8 unless `dup`
	int top_d[8], top_a[8], top_b[8];
};

// The part of ScoreBuffer::top1PE (src/ScoreBuffer.cpp:368-413) that does not depend on the running mean insert size: both candidate
// arrays sorted like the reference sorts them, the MAPQs, the candidates at or above best * pair_score_cutoff, and -- f(pair score,
// insert size, candidate of a, candidate of b) -- every combination inside the insert-size window in the order of the reference's
// double loop.  `a` = the mate whose scores arrive last (the odd read id: "read"), `b` = its mate.
// (NGM_HIP_HOST_TIMING: where pass 3's CPU time goes -- [0] ns in the two sorts, [1] ns in the rest of the walk, [2] candidates, [3] heads, [4] combinations looked at, [5] pairs)
inline std::atomic<bool> g_walk_probe{false};
inline std::atomic<uint64_t> g_walk_ns[6];
template <typename F>
static void walk_pair(const ngm_mapper_params &prm, uint32_t base_a, uint32_t cnt_a, int len_a, uint32_t base_b, uint32_t cnt_b, int len_b,
		const uint32_t *loc, const uint32_t *sv, const float *score, const uint32_t *rank, int *mq_a, int *mq_b, F &&f) {
	auto mq_of = [&](const uint32_t *v, uint32_t cnt) {  // computeMQ(MappedRead*), ScoreBuffer.cpp:42-49
		if (cnt <= 1) return 60;
		const float best = score[v[0]], second = score[v[1]];
		int mq = 0;
		if (best > 0 && second >= 0) mq = (int) ceilf(60.0f * (best - second) / best);
		return mq;
	};
	uint32_t small_a[32], small_b[32];  // nearly always enough; no allocation then
	std::vector<uint32_t> big_a, big_b;
	if (cnt_a > 32) big_a.resize(cnt_a);
	if (cnt_b > 32) big_b.resize(cnt_b);
	uint32_t *A = cnt_a > 32 ? big_a.data() : small_a, *B = cnt_b > 32 ? big_b.data() : small_b;
	const bool tm = g_walk_probe.load(std::memory_order_relaxed);
	const auto t_0 = tm ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
	sort_like_reference(A, base_a, cnt_a, loc, sv, score, rank);
	sort_like_reference(B, base_b, cnt_b, loc, sv, score, rank);
	const auto t_1 = tm ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
	struct WalkProbe { bool on; std::chrono::steady_clock::time_point t1; uint64_t cnt, *na, *nb, *nv; ~WalkProbe() { if (!on) return;
		g_walk_ns[1] += (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t1).count(); g_walk_ns[2] += cnt; g_walk_ns[3] += *na + *nb; g_walk_ns[4] += *nv; g_walk_ns[5] += 1; } };
	if (tm) g_walk_ns[0] += (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(t_1 - t_0).count();
	*mq_a = mq_of(A, cnt_a); *mq_b = mq_of(B, cnt_b);
	const float cutoff = prm.pair_score_cutoff > 0 ? prm.pair_score_cutoff : 0.9f;
	const float min_a = score[A[0]] * cutoff, min_b = score[B[0]] * cutoff;
	size_t na = 1, nb = 1;
	while (na < cnt_a && min_a <= score[A[na]]) ++na;
	while (nb < cnt_b && min_b <= score[B[nb]]) ++nb;
	uint64_t pna = na, pnb = nb, n_visits = 0;
	WalkProbe probe{tm, t_1, (uint64_t) cnt_a + cnt_b, &pna, &pnb, &n_visits};
	const int min_d = prm.min_insert_size, max_d = prm.max_insert_size > 0 ? prm.max_insert_size : INT_MAX;
	// Mates with hundreds of candidates each (repeat families of a GRCh38-like genome): CheckPairs walks all na x nb combinations,
	// but only those inside the insert-size window do anything -- B's candidates sorted by position, per candidate of A the ones
	// within max_d, visited in increasing j like the reference's inner loop: the same sequence of in-window pairs, so every
	// order-dependent outcome (first best, the equal counter, the recorded combinations) is unchanged.
	const bool windowed = na * nb > 1024 && max_d < (1 << 28);
	auto visit = [&](size_t i, size_t j) {
		++n_visits;
		const uint64_t l1 = loc[A[i]], l2 = loc[B[j]];
		const int cur = (int) ((l2 > l1) ? l2 - l1 + (uint64_t) len_b : l1 - l2 + (uint64_t) len_a);
		if (cur > min_d && cur < max_d) f(score[A[i]] + score[B[j]], cur, (int) A[i], (int) B[j]);
	};
	// (the reference's insert size is an `int` made from a 64-bit difference, ScoreBuffer.cpp:467-473: two locations at opposite ends of the
	// 32-bit range come out as a small number.  No genome ngm-hip accepts puts candidates there, but the window by location would miss what
	// the double loop counts: such lists take the double loop)
	bool wraps = false;
	if (windowed) {
		uint32_t l_min = 0xFFFFFFFFu, l_max = 0;
		for (size_t i = 0; i < na; ++i) { l_min = std::min(l_min, loc[A[i]]); l_max = std::max(l_max, loc[A[i]]); }
		for (size_t j = 0; j < nb; ++j) { l_min = std::min(l_min, loc[B[j]]); l_max = std::max(l_max, loc[B[j]]); }
		wraps = (uint64_t) (l_max - l_min) + (uint64_t) std::max(len_a, len_b) >= (1ull << 32);
	}
	if (!windowed || wraps) {
		for (size_t i = 0; i < na; ++i) for (size_t j = 0; j < nb; ++j) visit(i, j);
		return;
	}
	// Round 6 (the stress sub-leg of the bench: ~1 800 candidates above the cut-off per tied pair, 5 600 such pairs per batch): both heads
	// sorted by location, ONE sweep with two pointers gives every candidate of A its run of B's candidates within max_d -- the window's
	// bounds grow with the location -- and the double loop's order (i major, j ascending) comes from a bit per j: set for the run, read
	// back lowest first.  (Round 5: a binary search and a sort of the run per candidate of A -- half of pass 3's CPU time; sorting all
	// matches at once was tried and is slower: satellite arrays put hundreds of B's candidates into every window.)
	thread_local std::vector<uint64_t> a_by_loc, b_by_loc, bits;
	thread_local std::vector<uint32_t> run_lo, run_hi;
	a_by_loc.resize(na); b_by_loc.resize(nb); run_lo.resize(na); run_hi.resize(na);
	bits.assign((nb + 63) / 64, 0ull);
	for (size_t i = 0; i < na; ++i) a_by_loc[i] = ((uint64_t) loc[A[i]] << 32) | (uint64_t) i;
	for (size_t j = 0; j < nb; ++j) b_by_loc[j] = ((uint64_t) loc[B[j]] << 32) | (uint64_t) j;
	std::sort(a_by_loc.begin(), a_by_loc.end());
	std::sort(b_by_loc.begin(), b_by_loc.end());
	size_t lo = 0, hi = 0;
	for (size_t x = 0; x < na; ++x) {
		const uint64_t l1w = a_by_loc[x] >> 32;
		const uint64_t lo_loc = l1w > (uint64_t) max_d ? l1w - (uint64_t) max_d : 0u;
		const uint64_t hi_loc = std::min<uint64_t>(l1w + (uint64_t) max_d, 0xFFFFFFFFull);
		while (lo < nb && (b_by_loc[lo] >> 32) < lo_loc) ++lo;
		if (hi < lo) hi = lo;
		while (hi < nb && (b_by_loc[hi] >> 32) <= hi_loc) ++hi;
		const size_t i = (size_t) (a_by_loc[x] & 0xFFFFFFFFull);
		run_lo[i] = (uint32_t) lo; run_hi[i] = (uint32_t) hi;
	}
	for (size_t i = 0; i < na; ++i) {
		const uint32_t r0 = run_lo[i], r1 = run_hi[i];
		if (r1 - r0 == 1u) { visit(i, (size_t) (b_by_loc[r0] & 0xFFFFFFFFull)); continue; }
		if (r1 == r0) continue;
		uint32_t w_min = 0xFFFFFFFFu, w_max = 0;
		for (uint32_t y = r0; y < r1; ++y) {
			const uint32_t j = (uint32_t) b_by_loc[y], w = j >> 6;
			bits[w] |= 1ull << (j & 63u);
			w_min = std::min(w_min, w); w_max = std::max(w_max, w);
		}
		for (uint32_t w = w_min; w <= w_max; ++w) {
			uint64_t word = bits[w];
			bits[w] = 0ull;
			while (word) { visit(i, (size_t) w * 64u + (size_t) __builtin_ctzll(word)); word &= word - 1ull; }
		}
	}
}

// One pair's in-window combinations in the reference's order (walk_pair), kept: ScoreBuffer::CheckPairs at a given running mean
// is then a scan over them -- the sequential pass evaluates an open pair in microseconds instead of sorting and windowing again.
struct PairSeq {
	std::vector<float> ps;
	std::vector<int> d, a, b;
	int mq_a = 0, mq_b = 0;
};
// what build_seq hands walk_pair: a combination is kept unless eval_pair_seq passes over it whatever the running mean -- its `top` is the
// maximum of the pair scores so far, starting at 0, and a combination below it takes neither branch (a pair of two satellite-array
// mates has hundreds of thousands of those)
struct PairSeqKeeper {
	PairSeq &sq;
	float top = 0.0f;
	void operator()(float ps, int cur, int ia, int ib) {
		if (ps < top) return;
		top = ps;
		sq.ps.push_back(ps); sq.d.push_back(cur); sq.a.push_back(ia); sq.b.push_back(ib);
	}
};
struct PairOutcome { int wa, wb, mqa, mqb, equal, dist; bool found; };
// the double loop of top1PE over CheckPairs (src/ScoreBuffer.cpp:405-413, :463-502) at running mean `avg`
static PairOutcome eval_pair_seq(const PairSeq &q, int avg) {
	float top = 0.0f;
	int distance = 0, equal = 0, ta = -1, tb = -1;
	const size_t nq = q.ps.size();
	for (size_t x = 0; x < nq; ++x) {
		const float ps = q.ps[x];
		const int cur = q.d[x];
		bool take = false;
		if (ps > top * 1.00f) { top = ps; distance = cur; take = true; }
		else if (ps == top) {
			if (abs(distance - avg) > abs(cur - avg)) { top = ps; distance = cur; take = true; }
			else if (abs(distance) == abs(cur)) equal += 1;
		}
		if (take) { ta = q.a[x]; tb = q.b[x]; }
	}
	PairOutcome o{-1, -1, q.mq_a, q.mq_b, 0, 0, top > 0.0f};
	if (o.found) { o.wa = ta; o.wb = tb; o.equal = equal; o.dist = distance; }
	return o;
}

// ScoreBuffer::top1PE + CheckPairs (src/ScoreBuffer.cpp:368-502) for one pair; `a` = the mate whose scores arrive last
// (the odd read id: "read"), `b` = its mate.  Candidates are (pair index) lists into loc/score.
static void select_pair(const ngm_mapper_params &prm, const long dist_sum, const long dist_count, int *dist_out, uint32_t base_a, uint32_t cnt_a, int len_a, uint32_t base_b, uint32_t cnt_b, int len_b,
		const uint32_t *loc, const uint32_t *sv, const float *score, const uint32_t *rank, int *win_a, int *win_b, int *mq_a, int *mq_b, int *equal_out, bool *found,
		PairTies *ties = nullptr) {
	if (ties) *ties = PairTies{};
	if (cnt_a == 1 && cnt_b == 1) {  // the common case: one candidate per mate
		*mq_a = *mq_b = 60;
		const uint64_t l1 = loc[base_a], l2 = loc[base_b];
		const int cur = (int) ((l2 > l1) ? l2 - l1 + (uint64_t) len_b : l1 - l2 + (uint64_t) len_a);
		const int min_d1 = prm.min_insert_size, max_d1 = prm.max_insert_size > 0 ? prm.max_insert_size : INT_MAX;
		const float ps = score[base_a] + score[base_b];
		*found = cur > min_d1 && cur < max_d1 && ps > 0.0f;
		if (*found) { *dist_out = cur; *win_a = (int) base_a; *win_b = (int) base_b; *equal_out = 0; }
		return;
	}
	const int min_d = prm.min_insert_size, max_d = prm.max_insert_size > 0 ? prm.max_insert_size : INT_MAX;
	float top = 0.0f;
	int distance = 0, equal = 0, ta = -1, tb = -1, n_combo = 0;
	float combo_s[64];  // pair score, insert size and candidates of every pair inside the insert-size window
	int combo_d[64], combo_a[64], combo_b[64];
	const int avg = (int) (dist_sum / std::max(1L, dist_count));
	walk_pair(prm, base_a, cnt_a, len_a, base_b, cnt_b, len_b, loc, sv, score, rank, mq_a, mq_b, [&](float ps, int cur, int ia, int ib) {
		if (n_combo < 64) { combo_s[n_combo] = ps; combo_d[n_combo] = cur; combo_a[n_combo] = ia; combo_b[n_combo] = ib; }
		++n_combo;
		bool take = false;
		if (ps > top * 1.00f) { top = ps; distance = cur; take = true; }
		else if (ps == top) {
			if (abs(distance - avg) > abs(cur - avg)) { top = ps; distance = cur; take = true; }
			else if (abs(distance) == abs(cur)) equal += 1;
		}
		if (take) { ta = ia; tb = ib; }
	});
	*found = top > 0.0f;
	if (*found) { *dist_out = distance; *win_a = ta; *win_b = tb; *equal_out = equal; }
	// Which state does the outcome depend on besides the scores?  CheckPairs consults the running mean insert size (the
	// sequential state of the reference's CS thread) only when a pair's score equals the best so far, keeping the pair
	// closer to the mean; and it counts a pair as "equal" (NH / X0, never reset) when it ties with the current best in
	// score AND insert size.  So: no two in-window pairs of equal score -> the result is fixed.  Otherwise the winner is
	// the best-scoring pair closest to the mean, whatever the order, provided no two pairs share score and insert size
	// (`dup`: the first one in candidate order wins, later ones are counted) and the closest one is unique.
	if (ties && n_combo > 1) {
		if (n_combo > 64) { ties->equal_scores = ties->dup = true; ties->unique_closest = false; ties->dmin_top = min_d; ties->dmax_top = max_d; return; }
		int best_c = INT_MAX, n_best_c = 0, dmin = INT_MAX, dmax = 0;
		for (int x = 0; x < n_combo; ++x) {
			if (combo_s[x] == top) {
				const int cx = abs(combo_d[x] - avg);
				if (cx < best_c) { best_c = cx; n_best_c = 1; } else if (cx == best_c) ++n_best_c;
				dmin = std::min(dmin, combo_d[x]); dmax = std::max(dmax, combo_d[x]);
				if (*found) {
					if (ties->n_top < 8) { ties->top_d[ties->n_top] = combo_d[x]; ties->top_a[ties->n_top] = combo_a[x]; ties->top_b[ties->n_top] = combo_b[x]; }
					++ties->n_top;
				}
			}
			for (int y = x + 1; y < n_combo; ++y) if (combo_s[x] == combo_s[y]) { ties->equal_scores = true; if (combo_d[x] == combo_d[y]) ties->dup = true; }
		}
		ties->unique_closest = n_best_c <= 1;
		if (*found) { ties->dmin_top = dmin; ties->dmax_top = dmax; }
		if (ties->n_top > 8) ties->dup = true;  // too many to list: left to the exact sequential pass
	}
}
