// snp_device.h -- the kernels of `ngm-hip --snp` (csrc/snp.cpp; the walk, the counters' layout and the call rule: csrc/snp.h).
//
//   snp_add_kernel<Source>   one thread per alignment.  It issues the +1 / -1 pair of every covered block into the difference array (the
//                            walk of cov_add_kernel), then walks the aligned segments over the record's bases: the reference a dword (8
//                            bases) at a time, one no-return atomic add per mismatching, qualifying column and nothing per matching column.
//                            SnpArrays: what ngm_snp_add uploads.  SnpBatch: the mapper's own batch in place -- ngm_hit, SamRef, the CIGAR
//                            byte stream, the read and quality rows, read as the record formatter reads them (a reverse hit's row backwards
//                            and complemented) -- with cov::mapped_records_of_unit's decision which reads count.
//   the finish, per chunk    rocPRIM's inclusive scan over the chunk of the difference array (in place, the depth carried in),
//                            snp_flag_kernel (one thread per slot: reference class, the three counters, the call rule), rocPRIM's select of
//                            the flagged offsets, then snp_lengths_kernel / exclusive prefix / snp_write_kernel: the lines of the chunk's
//                            calls, with sam_u64 and the two sinks of sam_device.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coverage_device.h"
#include "snp.h"

namespace ngm {
namespace snp {

struct SnpArrays {
	const int32_t *ref_id, *pos0;
	const uint32_t *cigar_off;   // [n + 1]
	const char *cigar;
	const uint32_t *seq_off;     // [n + 1]
	const char *seq, *qual;      // qual: the same offsets, or null
	uint32_t n;
	struct Rec {
		int contig; int64_t pos0; const char *cigar; uint32_t cigar_len, seq_len;
		const char *seq, *qual;
		__device__ __forceinline__ char base(uint32_t i) const { return seq[i]; }
		__device__ __forceinline__ bool qual_ok(uint32_t i, int min_qual) const { return !qual || (int) (unsigned char) qual[i] - 33 >= min_qual; }
	};
	__device__ __forceinline__ uint32_t threads() const { return n; }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const uint32_t o = cigar_off[t], so = seq_off[t];
		f(Rec{(int) ref_id[t], (int64_t) pos0[t], cigar + o, cigar_off[t + 1] - o, seq_off[t + 1] - so, seq + so, qual ? qual + so : nullptr});
	}
};

struct SnpBatch {
	SamArgs A;
	int units;
	struct Rec {
		int contig; int64_t pos0; const char *cigar; uint32_t cigar_len, seq_len;
		const uint8_t *row, *q;
		int L, s0, QL;      // QL < 0: the read has no quality string
		bool reverse;
		int mate;           // 1: the second read of a pair (flag 0x80)
		// the printed sequence and qualities of bam_mapped / sam_mapped (sam_device.h)
		__device__ __forceinline__ char base(uint32_t i) const {
			if (!reverse) return (char) row[s0 + (int) i];
			const char ch = (char) row[L - 1 - (s0 + (int) i)];
			return ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch;
		}
		__device__ __forceinline__ bool qual_ok(uint32_t i, int min_qual) const {
			if (QL < 0) return true;
			const int at = reverse ? QL - 1 - (s0 + (int) i) : s0 + (int) i;
			const char qc = (at >= 0 && at < QL) ? (char) q[at] : ':';
			return (int) (unsigned char) qc - 33 >= min_qual;
		}
	};
	__device__ __forceinline__ uint32_t threads() const { return (uint32_t) units; }
	template <typename F> __device__ __forceinline__ void each(uint32_t t, F f) const {
		const uint32_t mask = cov::mapped_records_of_unit(A, (int) t);
		const int per = A.paired ? 2 : 1;
		for (int k = 0; k < per; ++k) {
			if (!((mask >> k) & 1u)) continue;
			const SamView v = sam_view(A, per * (int) t + k);
			const ngm_hit &h = *v.h;
			const SamRef rf = A.refs[v.i];
			const bool clip = A.hard_clip || A.silent_clip;
			const int s0 = max(0, min(clip ? (int) h.qstart : 0, v.L));
			const int sl = max(0, min(clip ? v.L - (int) h.qstart - (int) h.qend : v.L, v.L - s0));   // (never past the row)
			const int qlen = v.m.qual_len & 0x7FFF;
			f(Rec{h.contig, (int64_t) h.pos, A.str + rf.cig_off, (uint32_t) rf.cig_len, (uint32_t) sl, v.row, v.qual, v.L, s0, qlen ? min(qlen, v.L) : -1, h.reverse != 0, k});
		}
	}
};

// where an add kernel adds: the run's counters and the packed reference
struct Target {
	int32_t *diff;               // coverage.h's difference array
	uint32_t *alt;               // three per slot
	const uint64_t *off;         // [n_ref + 1] the contigs' offsets in the counter arrays
	const uint32_t *genome;      // 4-bit classes, 8 per dword
	const uint64_t *start;       // [n_ref] base offset of a contig in genome
	int n_ref, min_qual;
	unsigned long long *tot;     // [0] alignments [1] mismatching bases counted
};

template <typename Source>
__global__ __launch_bounds__(256) void snp_add_kernel(Source S, Target T) {
	__shared__ unsigned int s_n[2];
	if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mine = 0, counted = 0;
	if (t < S.threads()) {
		S.each(t, [&](const auto &rec) {
			if (rec.contig < 0 || rec.contig >= T.n_ref || rec.pos0 < 0) return;   // (never from the validated arrays; the mapper's records have a contig)
			++mine;
			const uint64_t base = T.off[rec.contig];
			const int64_t contig_len = (int64_t) (T.off[rec.contig + 1] - base - 1);
			cov::walk_cigar(rec.pos0, rec.cigar, rec.cigar_len, contig_len, [&](int64_t b, int64_t e) {
				atomicAdd(T.diff + base + (uint64_t) b, 1);   // (the results are not used: no-return atomics)
				atomicAdd(T.diff + base + (uint64_t) e, -1);
			});
			const uint64_t g0 = T.start[rec.contig];
			uint64_t w_at = ~0ull;
			uint32_t w = 0;
			walk_segments(rec.pos0, rec.cigar, rec.cigar_len, contig_len, [&](int64_t b, int64_t e, uint64_t ri) {
				for (int64_t p = b; p < e && ri < (uint64_t) rec.seq_len; ++p, ++ri) {   // (a validated record never runs out of bases)
					const uint64_t g = g0 + (uint64_t) p;
					if ((g >> 3) != w_at) { w_at = g >> 3; w = T.genome[w_at]; }
					const uint32_t r = (w >> (4u * (uint32_t) (g & 7u))) & 15u, c = read_class_of(rec.base((uint32_t) ri));
					if (r > 3u || c > 3u || c == r) continue;
					if (!rec.qual_ok((uint32_t) ri, T.min_qual)) continue;
					atomicAdd(T.alt + 3u * (base + (uint64_t) p) + alt_slot(c, r), 1u);
					++counted;
				}
			});
		});
	}
	if (mine) atomicAdd(&s_n[0], mine);
	if (counted) atomicAdd(&s_n[1], counted);
	__syncthreads();
	if (threadIdx.x < 2 && s_n[threadIdx.x]) atomicAdd(&T.tot[threadIdx.x], (unsigned long long) s_n[threadIdx.x]);
}

#ifdef NGM_SNP_FINISH_KERNELS   // (snp.cpp)
// a chunk of n slots at array offset s0; depth: its scanned difference array; alt: the chunk's counters
struct ChunkArgs {
	const int32_t *depth;
	const uint32_t *alt;
	uint32_t n;
	uint64_t s0;
	const uint64_t *off;       // [n_ref + 1]
	int n_ref;
	const uint32_t *genome;
	const uint64_t *start;
	Rule rule;
	uint8_t *flag;             // [n] the flag kernel's answer
	const uint32_t *idx;       // [m] chunk offsets of the calls, ascending
	uint32_t m;
	const char *names;         // the contigs' names, concatenated
	const uint32_t *name_off;  // [n_ref + 1]
	uint32_t *len;             // [m] pass 1
	const uint64_t *line_off;  // [m] exclusive prefix sums
	char *out;
	unsigned long long *totals;  // [0] calls [1] text bytes [2] covered bases
};

// the call at chunk offset i: its count (0: none), with the contig, the position in it, the reference class and the alternative's
__device__ __forceinline__ uint32_t snp_call_at(const ChunkArgs &T, uint32_t i, int *contig, uint64_t *pos, uint32_t *r, uint32_t *a) {
	const uint64_t g = T.s0 + i;
	const int c = cov::contig_of(T.off, T.n_ref, g);
	const uint64_t p = g - T.off[c];
	if (p + 1 >= T.off[c + 1] - T.off[c]) return 0;   // the contig's trailing slot
	const uint32_t cls = packed_class(T.genome, T.start[c] + p);
	if (cls > 3u) return 0;
	const uint32_t k[3] = {T.alt[3u * (uint64_t) i], T.alt[3u * (uint64_t) i + 1], T.alt[3u * (uint64_t) i + 2]};
	*contig = c; *pos = p; *r = cls;
	return call_of((int64_t) T.depth[i], cls, k, T.rule, a);
}

__global__ __launch_bounds__(256) void snp_flag_kernel(ChunkArgs T) {
	__shared__ unsigned long long s_cov;
	if (threadIdx.x == 0) s_cov = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < T.n) {
		int c; uint64_t p; uint32_t r, a;
		T.flag[i] = snp_call_at(T, i, &c, &p, &r, &a) ? 1 : 0;
		const int32_t d = T.depth[i];   // (0 on a trailing slot)
		if (d > 0) atomicAdd(&s_cov, (unsigned long long) d);
	}
	__syncthreads();
	if (threadIdx.x == 0 && s_cov) atomicAdd(&T.totals[2], s_cov);
}

template <typename Sink> __device__ __forceinline__ void snp_line(const ChunkArgs &T, uint32_t k, Sink &s) {
	const uint32_t i = T.idx[k];
	int c = 0; uint64_t p = 0; uint32_t r = 0, a = 0;
	const uint32_t n = snp_call_at(T, i, &c, &p, &r, &a);
	s.bytes(T.names + T.name_off[c], T.name_off[c + 1] - T.name_off[c]); s.put('\t');
	sam_u64(s, p + 1); sam_lit(s, "\t.\t"); s.put("ACGT"[r]); s.put('\t'); s.put("ACGT"[a]);
	sam_lit(s, "\t.\tPASS\tDP="); sam_u64(s, (unsigned long long) T.depth[i]); sam_lit(s, ";AO="); sam_u64(s, n); s.put('\n');
}

__global__ __launch_bounds__(256) void snp_lengths_kernel(ChunkArgs T) {
	__shared__ unsigned long long s_tot[2];
	if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < T.m) {
		SamCountSink s;
		snp_line(T, k, s);
		T.len[k] = s.n;
		atomicAdd(&s_tot[0], 1ull); atomicAdd(&s_tot[1], (unsigned long long) s.n);
	}
	__syncthreads();
	if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&T.totals[threadIdx.x], s_tot[threadIdx.x]);
}

__global__ __launch_bounds__(256) void snp_write_kernel(ChunkArgs T) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= T.m) return;
	SamWriteSink s{T.out + T.line_off[k]};
	snp_line(T, k, s);
}
#endif

}  // namespace snp
}  // namespace ngm
