// argos_device.h -- `--argos` on the GPU: every scored candidate of a read, ordered by score, as ScoreWriter's text line
// (src/ScoreBuffer.cpp:150-183 filter + std::sort(sortLocationScore), src/SequenceProvider.cpp:111-142 convert with the --argos
// clamp, src/writer/ScoreWriter.cpp:50-73 the line).
//
// Order classes of a read with survivors (candidates that pass --argos-min-score; all of them without a filter):
//   U  its positive scores are all distinct: the printed prefix (scores > 0, descending) does not depend on the input order of the sort;
//   S  at most 16 survivors and a tie among the positive scores: the reference's insertion sort is stable, the order is (score desc, rank asc)
//      with rank = the candidate's place in the reference's candidate list (candidate_order(), mapper_search.cpp);
//   H  more than 16 survivors and such a tie: libstdc++'s introsort is unstable -- the host runs that same std::sort over the survivors laid
//      out in rank order (mapper_argos.cpp).
// argos_order_kernel sorts the keys (score desc, secondary asc) of one read in LDS (bitonic, padded to a power of two): first with the
// candidate's index as secondary (classifies; final for U), then for the S reads again with their ranks.  Reads with more survivors than the
// LDS cap take the same sort over a slice of global memory, one workgroup per read (argos_order_kernel<true>).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngm {

constexpr int kArgosLdsCap = 1024;            // keys of one read in LDS (12 bytes each: key + candidate)
constexpr int kArgosThreadsLds = 64;          // one wave per read
constexpr int kArgosThreadsGlobal = 256;      // a workgroup per read of the long-list path
constexpr uint32_t kArgosRankUnknown = 0xFFFFFFFFu;   // = kCsOrderUnknown (cs_device.h)

enum : uint8_t { kArgosU = 0, kArgosS = 1, kArgosH = 2 };

struct ArgosArgs {
	int n;                        // reads of the batch (first pass) or entries of `list` (rank pass)
	const uint32_t *list;         // rank pass: the reads to order; null: read = blockIdx.x
	const uint32_t *cand_base, *cand_count;
	const float *scores;
	const uint16_t *read_len;
	const uint32_t *rank;         // null: secondary key = candidate index (first pass)
	float min_opt;                // --argos-min-score (<= 0: no filter)
	float match;                  // match bonus
	uint32_t lds_cap;             // reads with more candidates than this are left to the long-list path
	uint32_t lds_keys;            // keys the LDS holds: lds_cap rounded up to a power of two (dynamic LDS = 12 bytes each)
	const uint32_t *long_list;    // long-list path: its reads and their scratch slices (power-of-two sizes)
	const uint64_t *long_off;
	uint64_t *g_keys;
	uint32_t *g_vals;
	uint32_t *ord;                // [candidates] per read from cand_base on: the survivors' candidate indices, in print order
	uint32_t *n_surv, *n_pos;     // per read: survivors, survivors with a positive score
	uint8_t *cls;                 // per read: kArgosU / S / H
	unsigned long long *counters; // [0] reads whose S order fell back to positions (a rank unknown)
};

// float -> key that sorts ascending for DEScending scores
__host__ __device__ __forceinline__ uint32_t argos_desc_key(float s) {
	union { float f; uint32_t u; } b;
	b.f = s;
	const uint32_t u = b.u;
	const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
	return ~asc;
}

__device__ __forceinline__ float argos_min_score(const ArgosArgs &A, int read) {
	// ScoreBuffer.cpp:156-160: (length * match) * option when the option is at most 1, else the option
	return A.min_opt <= 1.0f ? __fmul_rn(__fmul_rn((float) A.read_len[read], A.match), A.min_opt) : A.min_opt;
}

template <bool kGlobal>
__global__ __launch_bounds__(kGlobal ? kArgosThreadsGlobal : kArgosThreadsLds) void argos_order_kernel(ArgosArgs A) {
	extern __shared__ uint64_t lds_keys[];
	__shared__ uint32_t s_cnt, s_pos, s_unknown, s_tie;
	const int B = kGlobal ? kArgosThreadsGlobal : kArgosThreadsLds;
	const uint32_t slot = blockIdx.x;
	if (!kGlobal && slot >= (uint32_t) A.n) return;
	const uint32_t read = kGlobal ? A.long_list[slot] : (A.list ? A.list[slot] : slot);
	const uint32_t base = A.cand_base[read], cnt = A.cand_count[read];
	if (!kGlobal && cnt > A.lds_cap) return;   // (the long-list launch takes it)
	if (cnt == 0) {
		if (threadIdx.x == 0) { A.n_surv[read] = 0; A.n_pos[read] = 0; A.cls[read] = kArgosU; }
		return;
	}
	uint32_t P = 1;
	while (P < cnt) P <<= 1;
	uint64_t *keys = kGlobal ? A.g_keys + A.long_off[slot] : lds_keys;
	uint32_t *vals = kGlobal ? A.g_vals + A.long_off[slot] : reinterpret_cast<uint32_t *>(lds_keys + A.lds_keys);
	if (threadIdx.x == 0) { s_cnt = 0; s_pos = 0; s_unknown = 0; s_tie = 0; }
	__syncthreads();
	const bool filter = A.min_opt > 0.0f;
	const float min = filter ? argos_min_score(A, (int) read) : 0.0f;
	bool use_rank = A.rank != nullptr;
	if (use_rank) {
		for (uint32_t x = threadIdx.x; x < cnt; x += B) if (A.rank[base + x] == kArgosRankUnknown) s_unknown = 1;
		__syncthreads();
		use_rank = s_unknown == 0;
	}
	// filter + compaction (the order of the survivors is irrelevant here: every key is distinct)
	for (uint32_t x = threadIdx.x; x < cnt; x += B) {
		const float s = A.scores[base + x];
		if (filter && !(s >= min)) continue;
		const uint32_t at = atomicAdd(&s_cnt, 1u);
		if (s > 0.0f) atomicAdd(&s_pos, 1u);
		const uint32_t sec = use_rank ? A.rank[base + x] : x;
		keys[at] = ((uint64_t) argos_desc_key(s) << 32) | sec;
		vals[at] = x;
	}
	__syncthreads();
	const uint32_t ns = s_cnt;
	for (uint32_t x = ns + threadIdx.x; x < P; x += B) { keys[x] = ~0ull; vals[x] = 0xFFFFFFFFu; }
	__syncthreads();
	// bitonic sort of P keys, ascending
	for (uint32_t k = 2; k <= P; k <<= 1) {
		for (uint32_t j = k >> 1; j > 0; j >>= 1) {
			for (uint32_t t = threadIdx.x; t < (P >> 1); t += B) {
				const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
				const uint64_t a = keys[i], b = keys[l];
				const bool up = (i & k) == 0;
				if ((a > b) == up) {
					keys[i] = b; keys[l] = a;
					const uint32_t va = vals[i]; vals[i] = vals[l]; vals[l] = va;
				}
			}
			__syncthreads();
		}
	}
	const uint32_t np = s_pos;
	for (uint32_t x = threadIdx.x; x < ns; x += B) {
		A.ord[base + x] = base + vals[x];
		if (x + 1 < np && (keys[x] >> 32) == (keys[x + 1] >> 32)) s_tie = 1;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		A.n_surv[read] = ns; A.n_pos[read] = np;
		if (!A.rank) A.cls[read] = s_tie ? (ns <= 16 ? kArgosS : kArgosH) : kArgosU;
		else if (!use_rank && A.counters) atomicAdd(A.counters, 1ull);
	}
}

// the H reads' order, computed on the host (libstdc++'s std::sort, mapper_argos.cpp): entries [hoff[j], hoff[j + 1]) of hord to ord[base ..)
__global__ __launch_bounds__(64) void argos_scatter_kernel(int n, const uint32_t *__restrict__ list, const uint32_t *__restrict__ hoff,
		const uint32_t *__restrict__ hord, const uint32_t *__restrict__ cand_base, uint32_t *__restrict__ ord) {
	const int j = blockIdx.x;
	if (j >= n) return;
	const uint32_t base = cand_base[list[j]], b = hoff[j], e = hoff[j + 1];
	for (uint32_t x = b + threadIdx.x; x < e; x += blockDim.x) ord[base + (x - b)] = hord[x];
}

// ---- the text: ScoreWriter::DoWriteReadGeneric (ScoreWriter.cpp:50-73) -----------------------------------------------------------
struct ArgosText {
	int n;
	const uint32_t *cand_base, *n_surv, *n_pos, *ord, *loc, *sv;
	const float *scores;
	const char *names;
	const uint32_t *meta;           // ngm_sam_read as two words: [0] name_off, [1] name_len | qual_len << 16
	const uint64_t *starts;         // contig starts + the artificial upper bound (n_contigs + 1 entries)
	int n_starts;
	uint32_t *len, *off;            // per read
	char *out;
	unsigned long long *counters;   // [0] reads with a line [1] entries written [2] 64-bit sum of the lengths
};

struct ArgosCount { uint32_t n = 0; __device__ void put(char) { ++n; } };
struct ArgosWrite { char *p; __device__ void put(char c) { *p++ = c; } };

template <typename Sink> __device__ __forceinline__ void argos_u32(Sink &s, uint32_t v) {
	char b[12];
	int i = 12;
	do { b[--i] = (char) ('0' + v % 10u); v /= 10u; } while (v);
	for (; i < 12; ++i) s.put(b[i]);
}
template <typename Sink> __device__ __forceinline__ void argos_i32(Sink &s, int v) {
	if (v < 0) { s.put('-'); argos_u32(s, 0u - (uint32_t) v); } else argos_u32(s, (uint32_t) v);
}

template <typename Sink> __device__ __forceinline__ void argos_line(const ArgosText &T, int i, Sink &s, uint32_t &entries) {
	const uint32_t name_off = T.meta[2 * i], name_len = T.meta[2 * i + 1] & 0xFFFFu;
	for (uint32_t c = 0; c < name_len; ++c) s.put(T.names[name_off + c]);
	const uint32_t np = T.n_pos[i], base = T.cand_base[i];
	int last = 0;
	for (uint32_t k = 0; k < np; ++k) {
		const uint32_t c = T.ord[base + k];
		const uint64_t loc = T.loc[c];
		// SequenceProvider::convert: upper_bound over the starts; a position less than 1000 before the next start becomes position 0 of
		// that contig with --argos (beyond the last contig: the upper bound's index and position 0, as the reference computes it)
		int lo = 0, hi = T.n_starts;
		while (lo < hi) { const int mid = (lo + hi) >> 1; if (T.starts[mid] <= loc) lo = mid + 1; else hi = mid; }
		int contig;
		uint64_t pos;
		if (lo < T.n_starts && T.starts[lo] - loc < 1000) { contig = lo; pos = 0; }
		else { contig = lo > 0 ? lo - 1 : 0; pos = loc - T.starts[contig]; }
		const int cur = (int) T.scores[c];
		s.put('\t'); argos_i32(s, contig); s.put(':'); argos_u32(s, (uint32_t) pos); s.put(':'); s.put((T.sv[c] & 1u) ? '1' : '0'); s.put(':');
		const int d = last - cur;
		argos_i32(s, d < 0 ? -d : d);
		last = cur;
	}
	s.put('\n');
	entries = np;
}

__global__ __launch_bounds__(256) void argos_lengths_kernel(ArgosText T) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= T.n) return;
	uint32_t len = 0, entries = 0;
	if (T.n_surv[i] > 0) {   // no survivor: unmapped, no line (ScoreWriter::DoWriteUnmappedRead writes nothing)
		ArgosCount c;
		argos_line(T, i, c, entries);
		len = c.n;
		atomicAdd(T.counters, 1ull);
		atomicAdd(T.counters + 1, (unsigned long long) entries);
		atomicAdd(T.counters + 2, (unsigned long long) len);
	}
	T.len[i] = len;
}

__global__ __launch_bounds__(256) void argos_write_kernel(ArgosText T) {
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= T.n || T.n_surv[i] == 0) return;
	ArgosWrite w{T.out + T.off[i]};
	uint32_t entries = 0;
	argos_line(T, i, w, entries);
}

}  // namespace ngm
