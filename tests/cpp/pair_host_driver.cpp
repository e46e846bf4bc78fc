// pair_host_driver.cpp -- the host-only pair logic (nextgenmap_amd/csrc/pair_host.h) for tests/test_pair_host.py, built with plain g++ and
// once more with -fsanitize=address,undefined:
//   pair_host_driver IN OUT   IN: records, each u32 kind + body; OUT: the results in the same order.  Every input array is copied into a
//                             heap block of exactly its length (a read past its end is the sanitizer's).
//   kind 1 (sort_like_reference + walk_pair) and kind 3 (select_pair):
//     u32 cnt_a, i32 len_a, u32 cnt_b, i32 len_b, u32 has_rank, f32 cutoff, i32 min_insert, i32 max_insert, u64 cap, i64 dist_sum, i64 dist_count,
//     then loc, sv (u32), score (f32) and -- with has_rank -- rank (u32), cnt_a + cnt_b entries each
//     kind 1 out: the two sorted lists, i32 mq_a, mq_b, u64 combinations, then of the first min(combinations, cap): f32 pair scores, i32 insert
//                 sizes, i32 candidates of a, i32 candidates of b
//     kind 3 out: i32 found, win_a, win_b, mq_a, mq_b, equal, dist (-1 where select_pair wrote nothing), then PairTies: i32 equal_scores, dup,
//                 unique_closest, dmin_top, dmax_top, n_top, and top_d, top_a, top_b of the first min(n_top, 8), zero filled to 8
//   kind 2 (eval_pair_seq on all combinations and on what PairSeqKeeper keeps): u64 n, i32 avg, then f32 pair scores, i32 insert sizes, a, b
//     out: i32 out_all[6], out_kept[6]: found, winner of a, of b, equal, insert size, combinations evaluated
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/pair_host.h"

static std::vector<uint8_t> slurp(const char *path) {
	std::vector<uint8_t> v;
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	uint8_t buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}

struct Reader {
	const std::vector<uint8_t> &in;
	size_t at = 0;
	template <typename T> T get() {
		T v;
		if (at + sizeof(T) > in.size()) { fprintf(stderr, "short input\n"); exit(2); }
		memcpy(&v, in.data() + at, sizeof(T));
		at += sizeof(T);
		return v;
	}
	template <typename T> std::unique_ptr<T[]> array(size_t n) {   // a block of exactly n entries
		if (at + n * sizeof(T) > in.size()) { fprintf(stderr, "short input\n"); exit(2); }
		std::unique_ptr<T[]> p(new T[n]);
		if (n) memcpy(p.get(), in.data() + at, n * sizeof(T));
		at += n * sizeof(T);
		return p;
	}
};

template <typename T>
static void put(std::string &s, T v) { s.append((const char *) &v, sizeof(T)); }
template <typename T>
static void put_all(std::string &s, const std::vector<T> &v) { s.append((const char *) v.data(), v.size() * sizeof(T)); }

static void walk_or_select(uint32_t kind, Reader &r, std::string &out) {
	const uint32_t cnt_a = r.get<uint32_t>(); const int len_a = r.get<int32_t>();
	const uint32_t cnt_b = r.get<uint32_t>(); const int len_b = r.get<int32_t>();
	const uint32_t has_rank = r.get<uint32_t>();
	ngm_mapper_params prm{};
	prm.pair_score_cutoff = r.get<float>(); prm.min_insert_size = r.get<int32_t>(); prm.max_insert_size = r.get<int32_t>();
	const uint64_t cap = r.get<uint64_t>();
	const long dist_sum = (long) r.get<int64_t>(), dist_count = (long) r.get<int64_t>();
	const size_t n = (size_t) cnt_a + cnt_b;
	const auto loc = r.array<uint32_t>(n), sv = r.array<uint32_t>(n);
	const auto score = r.array<float>(n);
	const auto rank = r.array<uint32_t>(has_rank ? n : 0);
	const uint32_t *rk = has_rank ? rank.get() : nullptr;
	int mq_a = -1, mq_b = -1;
	if (kind == 1) {
		std::vector<uint32_t> list_a(cnt_a), list_b(cnt_b);
		sort_like_reference(list_a.data(), 0, cnt_a, loc.get(), sv.get(), score.get(), rk);
		sort_like_reference(list_b.data(), cnt_a, cnt_b, loc.get(), sv.get(), score.get(), rk);
		std::vector<float> c_ps;
		std::vector<int32_t> c_d, c_a, c_b;
		uint64_t combos = 0;
		walk_pair(prm, 0, cnt_a, len_a, cnt_a, cnt_b, len_b, loc.get(), sv.get(), score.get(), rk, &mq_a, &mq_b, [&](float ps, int cur, int ia, int ib) {
			if (combos < cap) { c_ps.push_back(ps); c_d.push_back(cur); c_a.push_back(ia); c_b.push_back(ib); }
			++combos;
		});
		put_all(out, list_a); put_all(out, list_b);
		put<int32_t>(out, mq_a); put<int32_t>(out, mq_b); put<uint64_t>(out, combos);
		put_all(out, c_ps); put_all(out, c_d); put_all(out, c_a); put_all(out, c_b);
		return;
	}
	int dist = -1, win_a = -1, win_b = -1, equal = -1;
	bool found = false;
	PairTies ties;
	select_pair(prm, dist_sum, dist_count, &dist, 0, cnt_a, len_a, cnt_a, cnt_b, len_b, loc.get(), sv.get(), score.get(), rk, &win_a, &win_b, &mq_a, &mq_b, &equal, &found, &ties);
	for (int v : {found ? 1 : 0, win_a, win_b, mq_a, mq_b, equal, dist, ties.equal_scores ? 1 : 0, ties.dup ? 1 : 0, ties.unique_closest ? 1 : 0, ties.dmin_top, ties.dmax_top, ties.n_top})
		put<int32_t>(out, v);
	const int listed = ties.n_top < 8 ? ties.n_top : 8;
	for (const int *top : {ties.top_d, ties.top_a, ties.top_b}) for (int x = 0; x < 8; ++x) put<int32_t>(out, x < listed ? top[x] : 0);
}

static void eval(Reader &r, std::string &out) {
	const uint64_t n = r.get<uint64_t>();
	const int avg = r.get<int32_t>();
	const auto ps = r.array<float>(n);
	const auto d = r.array<int32_t>(n), a = r.array<int32_t>(n), b = r.array<int32_t>(n);
	PairSeq all, kept;
	PairSeqKeeper keep{kept};
	for (uint64_t x = 0; x < n; ++x) {
		all.ps.push_back(ps[x]); all.d.push_back(d[x]); all.a.push_back(a[x]); all.b.push_back(b[x]);
		keep(ps[x], d[x], a[x], b[x]);
	}
	for (const PairSeq *q : {&all, &kept}) {
		const PairOutcome o = eval_pair_seq(*q, avg);
		for (int v : {o.found ? 1 : 0, o.wa, o.wb, o.equal, o.dist, (int) q->ps.size()}) put<int32_t>(out, v);
	}
}

int main(int argc, char **argv) {
	if (argc != 3) { fprintf(stderr, "usage: pair_host_driver IN OUT\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[1]);
	Reader r{in};
	std::string out;
	while (r.at < in.size()) {
		const uint32_t kind = r.get<uint32_t>();
		if (kind == 1 || kind == 3) walk_or_select(kind, r, out);
		else if (kind == 2) eval(r, out);
		else { fprintf(stderr, "unknown record kind %u\n", kind); return 2; }
	}
	FILE *f = fopen(argv[2], "wb");
	if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
	return 0;
}
