// markdup.h -- the host-only parts of `ngm-hip --sort --markdup` (csrc/bam_sort.cpp, csrc/markdup_device.h): which records are examined, the
// unclipped 5' coordinate of a record, the end key and the pair key, the score of a record and the name comparison of two mates.  Compiles
// with plain g++ (tests/cpp/markdup_driver.cpp); every function is marked NGM_BS_HD: the kernels run the same code.
//
// The rules (INTEGRATION.md "Duplicate marking" states them too; tests/markdup_model.py is their executable form).  The result depends on
// the records and their run order (seq, position in the run) only.
//   Examined: flag 0x4, 0x100 and 0x800 clear and refID >= 0.  Every other record is never marked and never influences a decision.
//   u5, the unclipped 5' coordinate: forward strand (0x10 clear) pos minus the lengths of the leading S and H operations; reverse strand
//     record_end - 1 plus the lengths of the trailing S and H operations; clamped to [kU5Min, kU5Max] = [-2^30, 2^30 - 1] (pos and the end
//     are below 2^29 by the sorter's own refusal, clip lengths are bounded by nothing).  Without CIGAR operations u5 = pos.
//   End key: (refID, u5, strand), see end_key.
//   Pair: records g and g + 1 of the run order are mates when both are examined, both have 0x1, one has 0x40 and not 0x80, the other 0x80
//     and not 0x40, and their read names are byte-identical.  Mates with the first mate (0x40) in front form a pair.  Mates with the second
//     mate in front -- the order ngm-hip writes, as NextGenMap does -- form a pair unless one of the two is part of a pair of the first
//     kind with its other neighbour; so pairs never overlap, whatever the input.  Every other examined record is a fragment.  The first mate
//     of a pair is the record with 0x40; a pair's run-order index is that of its record in front.
//   Score: the sum of the quality bytes that are at least 15; 0 with absent qualities (first byte 0xFF) and with l_seq 0; a pair's score
//     is the sum of its mates'; 32 bits, saturating.
//   Pairs: grouped by pair key (see pair_key); the highest score survives, ties go to the lowest run-order index; both mates of every
//     other pair of the group get 0x400.
//   Fragments: grouped by end key together with both ends of every pair (survivor or not).  A group with a pair end: every fragment in
//     it gets 0x400.  Otherwise the highest score survives, ties to the lowest run-order index, the rest get 0x400.
//   The marker only ORs: a record that arrives with 0x400 keeps it and takes part like any other.
#pragma once

#include <cstddef>
#include <cstdint>

#include "bam_sort.h"

namespace ngm {
namespace markdup {

using bamsort::ld32;

constexpr int64_t kU5Min = -((int64_t) 1 << 30), kU5Max = ((int64_t) 1 << 30) - 1;
constexpr uint32_t kMinQual = 15;
constexpr uint64_t kNoKey = ~0ull;   // no end key and no half of a pair key has bit 63 set in its low word: this sorts behind all of them

// (p: a record check_record passed, here and below)
NGM_BS_HD inline uint32_t flag_of(const uint8_t *p) { return ld32(p + 16) >> 16; }

NGM_BS_HD inline bool examined(const uint8_t *p) { return (flag_of(p) & 0x904u) == 0 && (int32_t) ld32(p + 4) >= 0; }

NGM_BS_HD inline int64_t unclipped5(const uint8_t *p) {
	const int64_t pos = (int32_t) ld32(p + 8);
	const uint32_t n_cigar = ld32(p + 16) & 0xFFFFu;
	const uint8_t *c = p + 36 + p[12];
	int64_t u5;
	if (!(flag_of(p) & 0x10u)) {
		int64_t clip = 0;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t v = ld32(c + 4 * (size_t) k), op = v & 15u;
			if (op != 4 && op != 5) break;
			clip += v >> 4;
		}
		u5 = pos - clip;
	} else {
		int64_t clip = 0;
		for (uint32_t k = n_cigar; k > 0; --k) {
			const uint32_t v = ld32(c + 4 * (size_t) (k - 1)), op = v & 15u;
			if (op != 4 && op != 5) break;
			clip += v >> 4;
		}
		u5 = bamsort::record_end(p) - 1 + clip;
	}
	return u5 < kU5Min ? kU5Min : u5 > kU5Max ? kU5Max : u5;
}

// the end key: ((uint32) refID, u5 - kU5Min, reverse strand) ascending -- bits 62..32 refID (>= 0: 31 bits), 31..1 the biased u5 (31 bits),
// bit 0 the strand; bit 63 is clear
NGM_BS_HD inline uint64_t end_key(int32_t ref_id, int64_t u5, uint32_t flag) {
	return ((uint64_t) (uint32_t) ref_id << 32) | ((uint64_t) (u5 - kU5Min) << 1) | ((flag >> 4) & 1u);
}
NGM_BS_HD inline uint64_t end_key_of(const uint8_t *p) { return end_key((int32_t) ld32(p + 4), unclipped5(p), flag_of(p)); }

// the pair key of end keys e1 (first mate) and e2 (second mate): lo <= hi, the first mate's end first when they are equal; bit 63 of hi
// says that lo is the first mate's end, and only when both strands are equal -- FR and RF pairs do not tell the mates apart, FF and RR do
NGM_BS_HD inline void pair_key(uint64_t e1, uint64_t e2, uint64_t *lo, uint64_t *hi) {
	const bool first_is_lo = e1 <= e2, same_strand = ((e1 ^ e2) & 1u) == 0;
	*lo = first_is_lo ? e1 : e2;
	*hi = (first_is_lo ? e2 : e1) | ((uint64_t) (same_strand && first_is_lo ? 1u : 0u) << 63);
}

NGM_BS_HD inline uint32_t saturate32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) v; }
NGM_BS_HD inline uint32_t add_scores(uint32_t a, uint32_t b) { return saturate32((uint64_t) a + b); }

// where the qualities of a record start, and how many there are
NGM_BS_HD inline const uint8_t *qualities(const uint8_t *p, uint32_t *l_seq) {
	const uint32_t n = ld32(p + 20);
	*l_seq = n;
	return p + 36 + p[12] + 4 * (size_t) (ld32(p + 16) & 0xFFFFu) + ((size_t) n + 1) / 2;
}

NGM_BS_HD inline uint32_t record_score(const uint8_t *p) {
	uint32_t l_seq = 0;
	const uint8_t *q = qualities(p, &l_seq);
	if (l_seq == 0 || q[0] == 0xFF) return 0;
	uint64_t sum = 0;
	for (uint32_t i = 0; i < l_seq; ++i) if (q[i] >= kMinQual) sum += q[i];
	return saturate32(sum);
}

NGM_BS_HD inline bool same_name(const uint8_t *a, const uint8_t *b) {
	const uint32_t n = a[12];
	if (n != b[12]) return false;
	for (uint32_t i = 0; i < n; ++i) if (a[36 + i] != b[36 + i]) return false;
	return true;
}

// a, b: records g and g + 1 of the run order.  0: no mates; 1: mates, the first mate in front; 2: mates, the second mate in front
NGM_BS_HD inline int mates(const uint8_t *a, const uint8_t *b) {
	const uint32_t ra = flag_of(a) & 0xC1u, rb = flag_of(b) & 0xC1u;
	if (!((ra == 0x41u && rb == 0x81u) || (ra == 0x81u && rb == 0x41u))) return 0;
	if (!examined(a) || !examined(b) || !same_name(a, b)) return 0;
	return ra == 0x41u ? 1 : 2;
}

// whether records g and g + 1 (a, b) form a pair, with the records before and behind them (NULL at the ends of the run order): mates with
// the first mate in front always do, mates with the second mate in front unless a or b belongs to a pair of the first kind
NGM_BS_HD inline int pair_order(const uint8_t *prev, const uint8_t *a, const uint8_t *b, const uint8_t *next) {
	const int m = mates(a, b);
	if (m == 2 && ((prev && mates(prev, a) == 1) || (next && mates(b, next) == 1))) return 0;
	return m;
}

// what the arg-best of a group compares: the higher score wins, then the lower run-order index g (below 2^32 - 2).  Never 0, never ~0.
NGM_BS_HD inline uint64_t rank_of(uint32_t score, uint32_t g) { return ((uint64_t) score << 32) | (uint64_t) (0xFFFFFFFEu - g); }

}  // namespace markdup
}  // namespace ngm
