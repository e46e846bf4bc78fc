// methyl_device.h -- the kernels of `ngm-hip --bs-mapping --methyl` (csrc/methyl.cpp; the walk of a record, the context of a site and the
// file's definition: csrc/methyl.h).
//
//   methyl_add_kernel<Source>   one thread per alignment, running methyl.h's add_record with atomics for a sink (count_add_kernel's shape):
//                               the aligned segments are walked with the reference read a dword (8 bases) at a time, and a column over a
//                               reference C (top record) or G (bottom record) whose read base is a call costs one no-return device-scope
//                               atomic add.  MethylArrays: what ngm_methyl_add uploads (snp_device.h's SnpArrays and a bottom byte per
//                               alignment).  MethylBatch: the mapper's own batch in place (SnpBatch), a record's strand from its hit and
//                               from which mate it is.
//   the finish, per chunk       methyl_flag_kernel (one thread per base: reference class, the pair as one 8-byte load, depth rule, context,
//                               selection; the per-context sums reduced per block before they touch the totals), rocPRIM's select of the
//                               flagged offsets, then methyl_lengths_kernel / exclusive prefix / methyl_write_kernel: the lines of the
//                               chunk's sites, with sam_u64 and the two sinks of sam_device.h.  The neighbours come from the packed
//                               reference, which has no gap between contigs: the contig's bound comes from start[] and off[].
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "methyl.h"
#include "snp_device.h"

namespace ngm {
namespace met {

struct MethylArrays {
	snp::SnpArrays S;
	const uint8_t *bottom;   // [n]
	__device__ __forceinline__ uint32_t threads() const { return S.n; }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const bool bot = bottom[t] != 0;
		S.each(t, [&](const auto &rec) { f(rec, bot); });
	}
};

struct MethylBatch {
	snp::SnpBatch B;
	__device__ __forceinline__ uint32_t threads() const { return B.threads(); }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		B.each(t, [&](const auto &rec) { f(rec, rec.reverse != (rec.mate != 0)); });   // (the second mate of a pair: flag 0x80, sam_device.h's sam_unit)
	}
};

// where an add kernel adds
struct Counters {
	uint32_t *cnt;               // two per base: meth, unmeth
	unsigned long long *tot;     // [0] alignments
};

struct DeviceSink {
	uint32_t *cnt;
	__device__ __forceinline__ void add(uint64_t i) { atomicAdd(cnt + i, 1u); }   // (the result is not used: a no-return atomic)
};

template <typename Source>
__global__ __launch_bounds__(256) void methyl_add_kernel(Source S, Layout L, Counters C) {
	__shared__ unsigned int s_n;
	if (threadIdx.x == 0) s_n = 0;
	__syncthreads();
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mine = 0;
	if (t < S.threads()) {
		DeviceSink sink{C.cnt};
		S.each(t, [&](const auto &rec, bool bottom) {
			if (rec.contig < 0 || rec.contig >= L.n_ref || rec.pos0 < 0) return;
			uint32_t st[2];
			add_record(L, rec, bottom, sink, st);
			mine += 1u;
		});
	}
	if (mine) atomicAdd(&s_n, mine);
	__syncthreads();
	if (threadIdx.x == 0 && s_n) atomicAdd(&C.tot[0], (unsigned long long) s_n);
}

#ifdef NGM_METHYL_FINISH_KERNELS   // (methyl.cpp)
// a chunk of n bases at counter offset s0
struct ChunkArgs {
	const uint32_t *cnt;       // the run's counters (not the chunk's)
	uint32_t n;
	uint64_t s0;
	const uint64_t *off;       // [n_ref + 1]
	int n_ref;
	const uint32_t *genome;
	const uint64_t *start;
	uint32_t min_depth, selection;
	uint8_t *flag;             // [n] the flag kernel's answer
	const uint32_t *idx;       // [m] chunk offsets of the lines' sites, ascending
	uint32_t m;
	const char *names;         // the contigs' names, concatenated
	const uint32_t *name_off;  // [n_ref + 1]
	uint32_t *len;             // [m] pass 1
	const uint64_t *line_off;  // [m] exclusive prefix sums
	char *out;
	unsigned long long *totals;  // [0] lines [1..6] meth, unmeth of CG, CHG, CHH
};

// the site at chunk offset i: false when the base is neither C nor G; else its contig, position, class, counters, context and neighbours
struct Site { int contig; uint64_t pos; uint32_t cls, meth, unmeth, n[2]; int ctx; };
__device__ __forceinline__ bool methyl_site_at(const ChunkArgs &T, uint32_t i, Site *s) {
	const uint64_t g = T.s0 + i;
	const int c = cov::contig_of(T.off, T.n_ref, g);
	const uint64_t p = g - T.off[c], len = T.off[c + 1] - T.off[c];
	const uint32_t cls = snp::packed_class(T.genome, T.start[c] + p);
	if (cls != 1u && cls != 2u) return false;
	const uint2 pair = reinterpret_cast<const uint2 *>(T.cnt)[g];
	s->contig = c; s->pos = p; s->cls = cls; s->meth = pair.x; s->unmeth = pair.y;
	s->ctx = context_of(T.genome, T.start[c], len, p, cls, s->n);
	return true;
}

__global__ __launch_bounds__(256) void methyl_flag_kernel(ChunkArgs T) {
	__shared__ unsigned long long s_sum[6];
	if (threadIdx.x < 6) s_sum[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < T.n) {
		Site s;
		bool line = false;
		if (methyl_site_at(T, i, &s)) {
			line = is_line(s.meth, s.unmeth, s.ctx, T.min_depth, T.selection);
			if (s.ctx <= kCHH) {
				if (s.meth) atomicAdd(&s_sum[2 * s.ctx], (unsigned long long) s.meth);
				if (s.unmeth) atomicAdd(&s_sum[2 * s.ctx + 1], (unsigned long long) s.unmeth);
			}
		}
		T.flag[i] = line ? 1 : 0;
	}
	__syncthreads();
	if (threadIdx.x < 6 && s_sum[threadIdx.x]) atomicAdd(&T.totals[1 + threadIdx.x], s_sum[threadIdx.x]);
}

template <typename Sink> __device__ __forceinline__ void methyl_line(const ChunkArgs &T, uint32_t k, Sink &s) {
	Site x;
	if (!methyl_site_at(T, T.idx[k], &x)) return;   // (never: only sites are flagged)
	s.bytes(T.names + T.name_off[x.contig], T.name_off[x.contig + 1] - T.name_off[x.contig]); s.put('\t');
	sam_u64(s, x.pos + 1); s.put('\t'); s.put(x.cls == 1u ? '+' : '-'); s.put('\t'); sam_u64(s, x.meth); s.put('\t'); sam_u64(s, x.unmeth); s.put('\t');
	sam_lit(s, context_name(x.ctx)); s.put('\t'); s.put('C'); s.put("ACGTN"[x.n[0]]); s.put("ACGTN"[x.n[1]]); s.put('\n');
}

__global__ __launch_bounds__(256) void methyl_lengths_kernel(ChunkArgs T) {
	__shared__ unsigned long long s_lines;
	if (threadIdx.x == 0) s_lines = 0;
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < T.m) {
		SamCountSink s;
		methyl_line(T, k, s);
		T.len[k] = s.n;
		atomicAdd(&s_lines, 1ull);
	}
	__syncthreads();
	if (threadIdx.x == 0 && s_lines) atomicAdd(&T.totals[0], s_lines);
}

__global__ __launch_bounds__(256) void methyl_write_kernel(ChunkArgs T) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= T.m) return;
	SamWriteSink s{T.out + T.line_off[k]};
	methyl_line(T, k, s);
}
#endif

}  // namespace met
}  // namespace ngm
