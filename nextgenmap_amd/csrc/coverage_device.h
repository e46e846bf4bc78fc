// coverage_device.h -- the kernels of `ngm-hip --coverage` (csrc/coverage.cpp; the walk and the array's layout: csrc/coverage.h).
//
//   cov_add_kernel<Source>   one thread per alignment walks its CIGAR text and issues the two no-return atomic adds of every covered block
//                            (+1 at its begin, -1 at its end).  CovArrays: arrays of (ref_id, pos0, CIGAR offset) over a text blob, what
//                            ngm_coverage_add uploads.  CovBatch: the mapper's own batch in place -- ngm_hit, SamRef and the CIGAR / MD byte
//                            stream, the inputs sam_unit (sam_device.h) reads -- with sam_unit's decision which reads it writes as mapped records.
//   the finish, per chunk    rocPRIM's inclusive scan over the chunk's counters (in place, the depth carried in as its initial value),
//                            cov_heads_kernel (a slot is a run head when its depth differs from the slot before it), rocPRIM's select of the
//                            heads' offsets, then cov_lengths_kernel / exclusive prefix / cov_write_kernel: the lines of the chunk's runs,
//                            in the pattern of sam_lengths_kernel / sam_write_kernel and with their sam_u64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coverage.h"
#include "sam_device.h"

namespace ngm {
namespace cov {

struct CovArrays {
	const int32_t *ref_id, *pos0;
	const uint32_t *cigar_off;   // [n + 1]
	const char *text;
	uint32_t n;
	__device__ __forceinline__ uint32_t threads() const { return n; }
	// f(contig, pos0, cigar, cigar_len) for every alignment of thread t that counts
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const uint32_t o = cigar_off[t];
		f((int) ref_id[t], (int64_t) pos0[t], text + o, cigar_off[t + 1] - o);
	}
};

// which reads of a unit sam_unit writes as mapped records: bit 0 the unit's first read, bit 1 its second (GenericReadWriter::WriteRead /
// WritePair behind AlignmentBuffer::WriteRead, as sam_unit mirrors them -- the filters of sam_passes, the "no sequence" reads, the lost pairs)
__device__ __forceinline__ uint32_t mapped_records_of_unit(const SamArgs &A, int unit) {
	if (!A.paired) {
		const SamView v = sam_view(A, unit);
		if (v.m.qual_len & 0x8000u) return 0u;
		return sam_passes(A, v) ? 1u : 0u;
	}
	const SamView v1 = sam_view(A, 2 * unit), v2 = sam_view(A, 2 * unit + 1);
	if ((v1.m.qual_len & 0x8000u) || (v2.m.qual_len & 0x8000u)) return 0u;
	const ngm_hit &h1 = *v1.h, &h2 = *v2.h;
	if ((h1.pair_flags | h2.pair_flags) & NGM_PAIR_LOST) return 0u;
	bool paired_fail = (h1.pair_flags & NGM_PAIR_FAILED) || (h2.pair_flags & NGM_PAIR_FAILED);
	if (h1.mapped && h2.mapped) {
		const long long distance = (h2.pos > h1.pos) ? (long long) (h2.pos - h1.pos) + v1.L : (long long) (h1.pos - h2.pos) + v2.L;
		if (h1.contig != h2.contig || distance < A.min_insert || distance > A.max_insert || h1.reverse == h2.reverse) paired_fail = true;
	}
	const bool m1 = sam_passes(A, v1), m2 = sam_passes(A, v2);
	if (!m1 || !m2) return (m1 ? 1u : 0u) | (m2 ? 2u : 0u);
	if (!paired_fail && h1.reverse && h2.reverse) return 0u;   // (sam_unit writes nothing there)
	return 3u;
}

struct CovBatch {
	SamArgs A;
	int units;
	const uint64_t *off;   // the contigs' offsets, for their lengths
	__device__ __forceinline__ uint32_t threads() const { return (uint32_t) units; }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const uint32_t mask = mapped_records_of_unit(A, (int) t);
		const int per = A.paired ? 2 : 1;
		for (int k = 0; k < per; ++k) {
			if (!((mask >> k) & 1u)) continue;
			const int i = per * (int) t + k;
			const ngm_hit &h = A.hits[i];
			const SamRef rf = A.refs[i];
			f(h.contig, (int64_t) h.pos, A.str + rf.cig_off, (uint32_t) rf.cig_len);
		}
	}
};

// counters: the run's array; off: [n_ref + 1]; n_aln: alignments counted (one atomic per block)
template <typename Source>
__global__ __launch_bounds__(256) void cov_add_kernel(Source S, int32_t *counters, const uint64_t *off, int n_ref, unsigned long long *n_aln) {
	__shared__ unsigned int s_n;
	if (threadIdx.x == 0) s_n = 0;
	__syncthreads();
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mine = 0;
	if (t < S.threads()) {
		S.each(t, [&](int contig, int64_t pos0, const char *cigar, uint32_t len) {
			if (contig < 0 || contig >= n_ref || pos0 < 0) return;   // (never from the validated arrays; the mapper's records have a contig)
			++mine;
			const uint64_t base = off[contig];
			const int64_t contig_len = (int64_t) (off[contig + 1] - base - 1);
			walk_cigar(pos0, cigar, len, contig_len, [&](int64_t b, int64_t e) {
				atomicAdd(counters + base + (uint64_t) b, 1);   // (the results are not used: no-return atomics)
				atomicAdd(counters + base + (uint64_t) e, -1);
			});
		});
	}
	if (mine) atomicAdd(&s_n, mine);
	__syncthreads();
	if (threadIdx.x == 0 && s_n) atomicAdd(n_aln, (unsigned long long) s_n);
}

#ifdef NGM_COV_BATCH_KERNELS   // (mapper.cpp)
// the batch's decision alone, for a coverage object on another device: mask[unit] as mapped_records_of_unit says
__global__ __launch_bounds__(256) void cov_mask_kernel(SamArgs A, int units, uint8_t *mask) {
	const int u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u < units) mask[u] = (uint8_t) mapped_records_of_unit(A, u);
}
#endif

#ifdef NGM_COV_FINISH_KERNELS   // (coverage.cpp)
// depth: the scanned counters of the chunk; carry: the depth of the slot in front of it
__global__ __launch_bounds__(256) void cov_heads_kernel(const int32_t *depth, uint32_t n, int32_t carry, uint8_t *flag) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	flag[i] = depth[i] != (i ? depth[i - 1] : carry) ? 1 : 0;
}

// The runs that end in a chunk.  Run k in [0, m) begins at the head in front of it -- k = 0: the run carried in from the chunks before, at
// array offset open_off with depth open_depth; k > 0: at chunk offset head[k - 1] -- and ends at head[k].  It is a line when its depth is > 0.
struct TextArgs {
	const int32_t *depth;      // of the chunk
	const uint32_t *head;      // [m] chunk offsets of the heads, ascending
	uint32_t m;
	uint64_t s0;               // array offset of the chunk
	uint64_t open_off;
	int32_t open_depth;
	const uint64_t *off;       // [n_ref + 1]
	int n_ref;
	const char *names;         // the contigs' names, concatenated
	const uint32_t *name_off;  // [n_ref + 1]
	uint32_t *len;             // [m] pass 1
	const uint64_t *line_off;  // [m] exclusive prefix sums
	char *out;
	unsigned long long *totals;  // [0] covered bases [1] runs [2] text bytes
};

template <typename Sink> __device__ __forceinline__ bool cov_line(const TextArgs &T, uint32_t k, Sink &s, uint64_t *covered) {
	const uint64_t g0 = k ? T.s0 + T.head[k - 1] : T.open_off, g1 = T.s0 + T.head[k];
	const int32_t d = k ? T.depth[T.head[k - 1]] : T.open_depth;
	if (d <= 0) return false;
	const int c = contig_of(T.off, T.n_ref, g0);
	const uint64_t base = T.off[c];
	s.bytes(T.names + T.name_off[c], T.name_off[c + 1] - T.name_off[c]); s.put('\t');
	sam_u64(s, g0 - base); s.put('\t'); sam_u64(s, g1 - base); s.put('\t'); sam_u64(s, (unsigned long long) d); s.put('\n');
	*covered = (g1 - g0) * (uint64_t) d;
	return true;
}

__global__ __launch_bounds__(256) void cov_lengths_kernel(TextArgs T) {
	__shared__ unsigned long long s_tot[3];
	if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < T.m) {
		SamCountSink s;
		uint64_t covered = 0;
		const bool line = cov_line(T, k, s, &covered);
		T.len[k] = s.n;
		if (line) { atomicAdd(&s_tot[0], (unsigned long long) covered); atomicAdd(&s_tot[1], 1ull); atomicAdd(&s_tot[2], (unsigned long long) s.n); }
	}
	__syncthreads();
	if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(&T.totals[threadIdx.x], s_tot[threadIdx.x]);
}

__global__ __launch_bounds__(256) void cov_write_kernel(TextArgs T) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= T.m) return;
	SamWriteSink s{T.out + T.line_off[k]};
	uint64_t covered = 0;
	(void) cov_line(T, k, s, &covered);
}
#endif

}  // namespace cov
}  // namespace ngm
