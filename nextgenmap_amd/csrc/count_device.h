// count_device.h -- the kernels of `ngm-hip --count` (csrc/count.cpp; the tables, the walk of a record and the sums' definition: csrc/count.h).
//
//   count_add_kernel<Source>   one thread per alignment, running count.h's add_record with atomics for a sink.  A record whose span meets
//                              no merged interval returns after one binary search.  Otherwise the aligned segments are walked with the
//                              reference read a dword (8 bases) at a time: one no-return device-scope atomic add per eligible column inside an
//                              interval, a second one when the column is a conversion; then the regions the record overlaps get their
//                              reads / tc_reads atomics (64-bit), the per-column facts recomputed from the segment walk -- and only for a record
//                              that had a conversion at all.  CountArrays: what ngm_count_add uploads (snp_device.h's SnpArrays and a reverse
//                              byte per alignment).  CountBatch: the mapper's own batch in place (SnpBatch), a record's strand from its hit.
//   count_reduce_kernel        the finish: one wave per region.  The lanes stride over the region's slots -- reference class, mask bit, the
//                              slot's two counters as one 8-byte load -- and the four sums are reduced over the wave with shuffles.  The host
//                              formats the lines from the per-region array: regions are 10^5 at most, so there is no text kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "count.h"
#include "snp_device.h"

namespace ngm {
namespace cnt {

struct CountArrays {
	snp::SnpArrays S;
	const uint8_t *reverse;   // [n]
	__device__ __forceinline__ uint32_t threads() const { return S.n; }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const bool rev = reverse[t] != 0;
		S.each(t, [&](const auto &rec) { f(rec, rev); });
	}
};

struct CountBatch {
	snp::SnpBatch B;
	__device__ __forceinline__ uint32_t threads() const { return B.threads(); }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		B.each(t, [&](const auto &rec) { f(rec, rec.reverse); });
	}
};

// where an add kernel adds
struct Counters {
	uint32_t *cnt;               // two per slot: cov, conv
	unsigned long long *reg;     // two per region: reads, tc_reads
	unsigned long long *tot;     // [0] alignments [1] those a region took [2] eligible columns [3] conversions
};

struct DeviceSink {
	uint32_t *cnt; unsigned long long *reg;
	__device__ __forceinline__ void slot(uint64_t i) { atomicAdd(cnt + i, 1u); }   // (the results are not used: no-return atomics)
	__device__ __forceinline__ void region(uint64_t i) { atomicAdd(reg + i, 1ull); }
};

template <typename Source>
__global__ __launch_bounds__(256) void count_add_kernel(Source S, Layout L, Counters C) {
	__shared__ unsigned int s_n[4];
	if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mine[4] = {0, 0, 0, 0};
	if (t < S.threads()) {
		DeviceSink sink{C.cnt, C.reg};
		S.each(t, [&](const auto &rec, bool reverse) {
			if (rec.contig < 0 || rec.contig >= L.n_ref || rec.pos0 < 0) return;
			uint32_t st[3];
			add_record(L, rec, reverse, sink, st);
			mine[0] += 1u; mine[1] += st[0]; mine[2] += st[1]; mine[3] += st[2];
		});
	}
	for (int k = 0; k < 4; ++k) if (mine[k]) atomicAdd(&s_n[k], mine[k]);
	__syncthreads();
	if (threadIdx.x < 4 && s_n[threadIdx.x]) atomicAdd(&C.tot[threadIdx.x], (unsigned long long) s_n[threadIdx.x]);
}

#ifdef NGM_COUNT_FINISH_KERNELS   // (count.cpp)
struct ReduceArgs {
	const uint64_t *gbase;       // [n] where the region's first base lies in the packed reference
	const uint64_t *slot0;       // [n] the slot of its first base
	const uint32_t *len;         // [n]
	const uint8_t *take;         // [n]
	uint32_t n;
	const uint32_t *genome, *cnt, *mask;
	const unsigned long long *reg;
	long long *out;              // [n][6] t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads
};

__global__ __launch_bounds__(256) void count_reduce_kernel(ReduceArgs A) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t R = blockIdx.x * 4u + (threadIdx.x >> 6);   // (a wave has one region: it leaves as a whole)
	if (R >= A.n) return;
	const uint64_t g0 = A.gbase[R], s0 = A.slot0[R];
	const uint32_t len = A.len[R];
	const uint8_t take = A.take[R];
	const uint2 *pairs = reinterpret_cast<const uint2 *>(A.cnt);
	unsigned long long sum[4] = {0, 0, 0, 0};
	for (uint32_t i = lane; i < len; i += 64u) {
		if (!class_counts(take, snp::packed_class(A.genome, g0 + i))) continue;
		if (mask_bit(A.mask, s0 + i)) { sum[1] += 1ull; continue; }
		const uint2 c = pairs[s0 + i];
		sum[0] += 1ull; sum[2] += c.x; sum[3] += c.y;
	}
	for (int d = 32; d > 0; d >>= 1)
		for (int k = 0; k < 4; ++k) sum[k] += __shfl_down(sum[k], d, 64);
	if (lane == 0) {
		long long *o = A.out + 6ull * R;
		for (int k = 0; k < 4; ++k) o[k] = (long long) sum[k];
		o[4] = (long long) A.reg[2ull * R]; o[5] = (long long) A.reg[2ull * R + 1ull];
	}
}
#endif

}  // namespace cnt
}  // namespace ngm
