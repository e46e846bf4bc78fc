// markdup_device.h -- the kernels of `ngm-hip --sort --markdup` (csrc/bam_sort.cpp, mark_duplicates): end keys and pairs from the records
// in run order, the heads of the groups of equal keys in sorted order, the scores of the records whose group leaves something to decide,
// the arg-best of every group and the byte store of flag 0x400.  The rules: csrc/markdup.h; DESIGN.md section 4.
//
// g is a record's place in the run order, r a place in a sorted order.  Pairs live in slots: the pair of records g and g + 1 has slot
// g >> 1 (pairs do not overlap, so no two share a slot), which keeps them in run order without a scan.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "markdup.h"

namespace ngm {
namespace markdup {

// what a record is; a pair's record in front says which of the two is the first mate (0x40)
enum : uint8_t { kIgnored = 0, kFragment = 1, kHeadFirst = 2, kTail = 3, kHeadSecond = 4 };
__host__ __device__ inline bool is_head(uint8_t kind) { return kind == kHeadFirst || kind == kHeadSecond; }
// the counters: ngm_bam_sort_markdup_stats' six
enum { kExamined = 0, kPairs = 1, kFragments = 2, kDupPairs = 3, kDupFragments = 4, kNewlyMarked = 5, kCounters = 6 };

// every lane of the wave calls this: one atomic per wave
__device__ inline void wave_add(unsigned long long *ctr, uint32_t v) {
#pragma unroll
	for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
	if ((threadIdx.x & 63u) == 0 && v) atomicAdd(ctr, (unsigned long long) v);
}

// ORs 0x400 into the record at ptr: bit 2 of byte 19, the flag's high byte.  One thread owns a record.  True: the bit was clear.
__device__ inline bool mark(uint64_t ptr) {
	uint8_t *b = (uint8_t *) (uintptr_t) ptr + 19;
	const uint8_t v = *b;
	if (v & 4u) return false;
	*b = (uint8_t) (v | 4u);
	return true;
}

// the addresses of a segment's records, records g0 .. g0 + n of the run order
__global__ __launch_bounds__(256) void ptrs_kernel(const uint8_t *seg, const uint32_t *rec_off, uint32_t n, uint64_t g0, uint64_t *ptr) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n) ptr[g0 + i] = (uint64_t) (uintptr_t) (seg + rec_off[i]);
}

// One thread per record: what it is (ignored, fragment, in front or behind in a pair -- the pair test looks at up to two records before and
// two behind it) and its end key (kNoKey when ignored).  Reads the fixed part, the name and the CIGAR only: offsets the walk has validated.
__global__ __launch_bounds__(256) void ends_kernel(const uint64_t *ptr, uint64_t n, uint64_t *ek, uint8_t *kind, unsigned long long *counters) {
	const uint64_t g = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	uint8_t k = kIgnored;
	if (g < n) {
		const uint8_t *p = (const uint8_t *) (uintptr_t) ptr[g];
		uint64_t e = kNoKey;
		if (examined(p)) {
			const uint32_t role = flag_of(p) & 0xC1u;
			k = kFragment;
			if (role == 0x41u || role == 0x81u) {
				auto at = [&](uint64_t i) { return (const uint8_t *) (uintptr_t) ptr[i]; };
				const uint8_t *before = g > 0 ? at(g - 1) : nullptr, *behind = g + 1 < n ? at(g + 1) : nullptr;
				int o = behind ? pair_order(before, p, behind, g + 2 < n ? at(g + 2) : nullptr) : 0;
				if (o) k = o == 1 ? kHeadFirst : kHeadSecond;
				else if (before && pair_order(g > 1 ? at(g - 2) : nullptr, before, p, behind)) k = kTail;
			}
			e = end_key_of(p);
		}
		ek[g] = e;
		kind[g] = k;
	}
	wave_add(counters + kExamined, k != kIgnored);
	wave_add(counters + kPairs, is_head(k));
	wave_add(counters + kFragments, k == kFragment);
}

// the pair key of every pair into its slot (the slots without a pair keep kNoKey in both halves)
__global__ __launch_bounds__(256) void pair_keys_kernel(const uint64_t *ek, const uint8_t *kind, uint64_t n, uint64_t *lo, uint64_t *hi) {
	const uint64_t g = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (g >= n || !is_head(kind[g])) return;
	const bool first = kind[g] == kHeadFirst;
	pair_key(ek[first ? g : g + 1], ek[first ? g + 1 : g], lo + (g >> 1), hi + (g >> 1));
}

__global__ __launch_bounds__(256) void gather64_kernel(const uint32_t *idx, uint64_t n, const uint64_t *src, uint64_t *dst) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r < n) dst[r] = src[idx[r]];
}

// hp[r] = r where a group of equal keys (k1, and k2 when given) starts, else 0: an inclusive max-scan makes it the place of r's group head
__global__ __launch_bounds__(256) void heads_kernel(const uint64_t *k1, const uint64_t *k2, uint64_t n, uint32_t *hp) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	const bool head = r == 0 || k1[r] != k1[r - 1] || (k2 && k2[r] != k2[r - 1]);
	hp[r] = head ? (uint32_t) r : 0u;
}

// after the scan: r's group has more than one member
__device__ inline bool in_a_group(const uint32_t *hp, uint64_t r, uint64_t n) { return hp[r] != (uint32_t) r || (r + 1 < n && hp[r + 1] != (uint32_t) (r + 1)); }

// the record in front of the pair in a slot
__device__ inline uint64_t head_of(uint32_t slot, const uint8_t *kind) { const uint64_t g = (uint64_t) slot * 2u; return is_head(kind[g]) ? g : g + 1; }

// ---- scores ------------------------------------------------------------------------------------------------------------------------------
// A wave owns 64 consecutive records of the run order and takes those with need[g] set one after the other: the record's qualities as
// aligned dwords, one per lane and round (coalesced; a thread of its own per record would walk them byte by byte, 64 distant streams per
// wave), the bytes outside [q, q + l_seq) masked off, then a butterfly sum.  The aligned dwords may start up to 3 bytes before the
// qualities and end up to 3 bytes behind them: inside the segment, which is 256-byte aligned and ends with 16 bytes of padding.
__global__ __launch_bounds__(256) void scores_kernel(const uint64_t *ptr, uint64_t n, const uint8_t *need, uint32_t *score) {
	const uint64_t g = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	const bool mine = g < n && need[g];
	const unsigned long long my_ptr = mine ? ptr[g] : 0ull;
	unsigned long long todo = __ballot(mine);
	uint32_t my_score = 0;
	while (todo) {   // (the same for all lanes)
		const uint32_t j = (uint32_t) (__ffsll((long long) todo) - 1);
		todo &= todo - 1;
		const uint8_t *p = (const uint8_t *) (uintptr_t) __shfl(my_ptr, (int) j);
		uint32_t l_seq = 0;
		const uint8_t *q = qualities(p, &l_seq);
		unsigned long long sum = 0;
		if (l_seq != 0 && q[0] != 0xFF) {
			const uintptr_t a = (uintptr_t) q, a0 = a & ~(uintptr_t) 3, end = a + l_seq;
			const uint64_t n_dw = (end - a0 + 3) / 4;
			for (uint64_t d = lane; d < n_dw; d += 64) {
				const uintptr_t at = a0 + 4 * d;
				const uint32_t w = *(const uint32_t *) at;
#pragma unroll
				for (uint32_t b = 0; b < 4; ++b) {
					const uint32_t v = (w >> (8 * b)) & 0xFFu;
					if (at + b >= a && at + b < end && v >= kMinQual) sum += v;
				}
			}
		}
#pragma unroll
		for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
		if (lane == j) my_score = saturate32(sum);
	}
	if (mine) score[g] = my_score;
}

// ---- pairs: r over the first n sorted slots, the ones that hold a pair -----------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_need_kernel(const uint32_t *slot, const uint32_t *hp, uint64_t n, const uint8_t *kind, uint8_t *need) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n || !in_a_group(hp, r, n)) return;
	const uint64_t g = head_of(slot[r], kind);
	need[g] = 1; need[g + 1] = 1;
}

__global__ __launch_bounds__(256) void pair_best_kernel(const uint32_t *slot, const uint32_t *hp, uint64_t n, const uint8_t *kind, const uint32_t *score, unsigned long long *best) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n || !in_a_group(hp, r, n)) return;
	const uint64_t g = head_of(slot[r], kind);
	atomicMax(best + hp[r], (unsigned long long) rank_of(add_scores(score[g], score[g + 1]), (uint32_t) g));
}

__global__ __launch_bounds__(256) void pair_mark_kernel(const uint32_t *slot, const uint32_t *hp, uint64_t n, const uint8_t *kind, const uint32_t *score, const unsigned long long *best,
		const uint64_t *ptr, unsigned long long *counters) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	uint32_t dup = 0, fresh = 0;
	if (r < n && in_a_group(hp, r, n)) {
		const uint64_t g = head_of(slot[r], kind);
		if (best[hp[r]] != rank_of(add_scores(score[g], score[g + 1]), (uint32_t) g)) {
			dup = 1;
			fresh = (mark(ptr[g]) ? 1u : 0u) + (mark(ptr[g + 1]) ? 1u : 0u);
		}
	}
	wave_add(counters + kDupPairs, dup);
	wave_add(counters + kNewlyMarked, fresh);
}

// ---- fragments: r over the first n records sorted by end key, the examined ones ---------------------------------------------------------
// best[head of the group] = ~0 where the group holds an end of a pair (every writer stores the same value)
__global__ __launch_bounds__(256) void pair_ends_kernel(const uint32_t *idx, const uint32_t *hp, uint64_t n, const uint8_t *kind, unsigned long long *best) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r < n && kind[idx[r]] >= kHeadFirst) best[hp[r]] = ~0ull;
}

// a fragment whose group leaves something to decide by score: more than one member and no end of a pair
__device__ inline bool contested(const uint32_t *hp, uint64_t r, uint64_t n, uint8_t kind, const unsigned long long *best) {
	return kind == kFragment && in_a_group(hp, r, n) && best[hp[r]] != ~0ull;
}

__global__ __launch_bounds__(256) void frag_need_kernel(const uint32_t *idx, const uint32_t *hp, uint64_t n, const uint8_t *kind, const unsigned long long *best, uint8_t *need) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	const uint32_t g = idx[r];
	if (contested(hp, r, n, kind[g], best)) need[g] = 1;
}

__global__ __launch_bounds__(256) void frag_best_kernel(const uint32_t *idx, const uint32_t *hp, uint64_t n, const uint8_t *kind, const uint32_t *score, unsigned long long *best) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	const uint32_t g = idx[r];
	if (contested(hp, r, n, kind[g], best)) atomicMax(best + hp[r], (unsigned long long) rank_of(score[g], g));   // (a rank is never ~0)
}

__global__ __launch_bounds__(256) void frag_mark_kernel(const uint32_t *idx, const uint32_t *hp, uint64_t n, const uint8_t *kind, const uint32_t *score, const unsigned long long *best,
		const uint64_t *ptr, unsigned long long *counters) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	uint32_t dup = 0, fresh = 0;
	if (r < n) {
		const uint32_t g = idx[r];
		if (kind[g] == kFragment) {
			const unsigned long long b = best[hp[r]];
			if (b == ~0ull || (in_a_group(hp, r, n) && b != rank_of(score[g], g))) {
				dup = 1;
				fresh = mark(ptr[g]) ? 1u : 0u;
			}
		}
	}
	wave_add(counters + kDupFragments, dup);
	wave_add(counters + kNewlyMarked, fresh);
}

}  // namespace markdup
}  // namespace ngm
