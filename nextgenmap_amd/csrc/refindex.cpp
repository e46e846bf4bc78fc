// refindex.cpp -- reference encoding and k-mer index construction (host walk + GPU sort).
// See refindex.h for what it replaces and for the HBM layout.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "refindex.h"
#include "thread_pool.h"

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <zlib.h>

namespace ngm { long test_limit(const char *key, long dflt); }  // NGM_HIP_TEST_LIMITS (mapper_search.cpp)

namespace {
thread_local std::string g_pipeline_error;

#define REF_HIP_TRY(expr)                                                                      \
	do {                                                                                       \
		hipError_t e_ = (expr);                                                                \
		if (e_ != hipSuccess) {                                                                \
			ngm::pipeline_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return -5;                                                                         \
		}                                                                                      \
	} while (0)

using ngm::Buf;

inline uint8_t class_of_base(uint8_t c) {  // enc4 semantics (SequenceProvider.cpp:72-85): non-ACGT -> N
	switch (c & 0xDF) {
	case 'A': return 0;
	case 'C': return 1;
	case 'G': return 2;
	case 'T': return 3;
	default: return 5;
	}
}

// ---- the reference's k-mer enumeration, restated ---------------------------------------------------
// CS::PrefixIteration (src/CSstatic.cpp:26-76) with prefixskip = kmer_skip over one contig, feeding
// CompactPrefixTable::CountKmer / BuildPrefixTable (src/PrefixTable.cpp:641-709): emits the (k-mer,
// position) pairs that end up in the index, in genome order.
struct KmerWalker {
	int k, skip, bin_shift;
	uint32_t mask;
	uint32_t last_prefix;
	int64_t last_bin;
	std::vector<uint32_t> *keys, *vals;
	uint64_t visited = 0;

	void fire(uint32_t prefix, uint64_t pos) {
		++visited;
		// same k-mer as the previous indexed one AND same bin as the previous same-k-mer hit -> dropped
		if (prefix == last_prefix) {
			const int64_t bin = (int64_t) (pos >> bin_shift);
			if (bin != last_bin || last_bin == -1) { keys->push_back(prefix); vals->push_back((uint32_t) pos); }
			last_bin = bin;
		} else {
			last_bin = -1;
			keys->push_back(prefix);
			vals->push_back((uint32_t) pos);
		}
		last_prefix = prefix;
	}

	// seq: class per base, the reference's quirks already applied (see walk_contig); N = class 5
	void iterate(const uint8_t *seq, uint64_t length, uint64_t offset) {
		for (;;) {  // the reference recurses after every 'N'; this loop is that recursion
			if (length < (uint64_t) k) return;
			if (seq[0] == 5) {
				uint64_t n_skip = 1;
				while (n_skip < length && seq[n_skip] == 5) ++n_skip;
				seq += n_skip;
				if (n_skip >= (length - k)) return;  // CSstatic.cpp:37 (drops a tail of exactly k bases too)
				length -= n_skip;
				offset += n_skip;
			}
			uint32_t prefix = 0;
			bool restart = false;
			for (uint64_t i = 0; i < (uint64_t) k - 1; ++i) {
				if (seq[i] == 5) { seq += i + 1; length -= i + 1; offset += i + 1; restart = true; break; }
				prefix = (prefix << 2) | ngm::kmer_code_of_class(seq[i]);
			}
			if (restart) continue;
			int skipcount = skip;
			for (uint64_t i = k - 1; i < length; ++i) {
				if (seq[i] == 5) { seq += i + 1; length -= i + 1; offset += i + 1; restart = true; break; }
				prefix = ((prefix << 2) | ngm::kmer_code_of_class(seq[i])) & mask;
				if (skipcount == skip) { fire(prefix, offset + i + 1 - k); skipcount = 0; }
				else ++skipcount;
			}
			if (!restart) return;
		}
	}
};

__global__ void mark_runs_kernel(const uint32_t *__restrict__ keys, uint64_t n, uint32_t *__restrict__ starts, uint32_t *__restrict__ raw) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const uint32_t kj = keys[j];
	if (j == 0 || keys[j - 1] != kj) starts[kj] = (uint32_t) j;
	if (j + 1 == n || keys[j + 1] != kj) raw[kj] = (uint32_t) (j + 1);  // end; turned into a length below
}

__global__ void finish_index_kernel(uint32_t n_kmers, int k, const uint32_t *__restrict__ starts, uint32_t *__restrict__ raw,
		uint2 *__restrict__ index) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n_kmers) return;
	const uint32_t end = raw[p];
	const uint32_t cnt = end ? end - starts[p] : 0u;  // raw[] holds end+0 only for present k-mers
	raw[p] = cnt;
	index[p] = make_uint2(starts[p], cnt);
}

__device__ __forceinline__ uint32_t d_revcomp(uint32_t prefix, int k) {
	const int shift = 32 - 2 * k;
	uint32_t c = (prefix ^ 0xAAAAAAAAu) << shift;
	c = (c & 0xFFFF0000u) >> 16 | (c & 0x0000FFFFu) << 16;
	c = (c & 0xFF00FF00u) >> 8 | (c & 0x00FF00FFu) << 8;
	c = (c & 0xF0F0F0F0u) >> 4 | (c & 0x0F0F0F0Fu) << 4;
	c = (c & 0xCCCCCCCCu) >> 2 | (c & 0x33333333u) << 2;
	return c;
}

// the reference marks a k-mer unused when (10000 - min(total,10000)) * 100 / 10000 truncates to 0, i.e.
// total = own + reverse-complement occurrences >= 9901 (PrefixTable.cpp:468-478); lookups then see an empty list
__global__ void apply_usage_rule_kernel(uint32_t n_kmers, int k, const uint32_t *__restrict__ raw, uint2 *__restrict__ index) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n_kmers) return;
	const uint32_t total = raw[p] + raw[d_revcomp(p, k)];
	if (total > 9900u) index[p].y = 0;
}

void index_stats(ngm_ref *r, const uint32_t *raw, uint32_t n_kmers);
int upload_staged(void *dst, const void *src, size_t bytes);

// ---- the same enumeration on the GPU ------------------------------------------------------------------------
// KmerWalker above, position-parallel.  Which k-mers the reference visits (CS::PrefixIteration, src/CSstatic.cpp:26-76, with
// prefixskip = kmer_skip) follows from the N-free runs of a contig alone: in a maximal N-free run [a, b) the k-mers start at
// a, a + (skip+1), ... while start + k <= b (the skip counter restarts at every restart), except the run of exactly k bases at
// the contig end behind an N run that the walker meets at a restart position (CSstatic.cpp:37).  Which of them are stored
// (CompactPrefixTable::CountKmer / BuildPrefixTable, src/PrefixTable.cpp:641-709: a k-mer equal to the previously visited one is
// dropped when it falls into the same bin as that one, from the third of such a run on) depends on the two visited k-mers before
// it only.  So: N marks -> inclusive max-scan = start of the current run -> visit flags -> compaction -> keys -> store flags ->
// compaction; all in HBM (12.4 GB of scratch for a GRCh38-size genome).
__device__ __forceinline__ uint32_t d_class_at(const uint32_t *g, uint64_t i) { return (g[i >> 3] >> (4 * (int) (i & 7))) & 15u; }

__global__ void walk_mark_n_kernel(const uint32_t *__restrict__ genome, uint64_t n, uint32_t *__restrict__ v) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) v[i] = d_class_at(genome, i) == 5u ? (uint32_t) i + 1u : 0u;
}
// the last two bases of every contig act as 'A' for the walk (see build_index below)
__global__ void walk_unmark_tails_kernel(const uint64_t *__restrict__ cend, int n_contigs, uint32_t *__restrict__ v) {
	const int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < n_contigs) { v[cend[c] - 1] = 0; v[cend[c] - 2] = 0; }
}
__device__ __forceinline__ int walk_contig_of(const uint64_t *cstart, int n_contigs, uint64_t pos) {  // last contig with start <= pos
	int lo = 0, hi = n_contigs;
	while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (cstart[mid] <= pos) lo = mid; else hi = mid; }
	return lo;
}
__global__ void walk_visit_flags_kernel(const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ genome, uint64_t n, int k, int step,
		const uint64_t *__restrict__ cstart, const uint64_t *__restrict__ cend, int n_contigs, uint8_t *__restrict__ flag) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	uint8_t f = 0;
	if (i + k <= n) {
		const uint64_t a = run_start[i + k - 1];  // index after the last N at or before i + k - 1
		if (a <= i && (i - a) % (uint64_t) step == 0) {
			f = 1;
			if (i == a) {  // CSstatic.cpp:37: exactly k bases left behind an N run met at a restart position
				const int c = walk_contig_of(cstart, n_contigs, i);
				const uint64_t p = i - cstart[c];
				if (i + k == cend[c] && p >= 1 && d_class_at(genome, i - 1) == 5u && (p == 1 || d_class_at(genome, i - 2) == 5u)) f = 0;
			}
		}
	}
	flag[i] = f;
}
__global__ void walk_keys_kernel(const uint32_t *__restrict__ pos, uint64_t m, const uint32_t *__restrict__ genome, int k, const uint64_t *__restrict__ cstart,
		const uint64_t *__restrict__ cend, int n_contigs, uint32_t *__restrict__ keys) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint64_t p = pos[j];
	const uint64_t tail = cend[walk_contig_of(cstart, n_contigs, p)] - 2;  // from here on the walk sees 'A'
	uint32_t key = 0;
	for (int t = 0; t < k; ++t) {
		const uint32_t cls = (p + t >= tail) ? 0u : d_class_at(genome, p + t);
		key = (key << 2) | (cls == 2u ? 3u : (cls == 3u ? 2u : cls));  // A0 C1 T2 G3 (CSstatic.cpp:20-22)
	}
	keys[j] = key;
}
// PrefixTable.cpp:641-709 (fire() of the host walker): stored unless it repeats the previous visited k-mer of its contig in the
// same bin, where the bin memory starts with the second k-mer of such a run
__global__ void walk_store_flags_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ keys, uint64_t m, int bin_shift,
		const uint64_t *__restrict__ cstart, int n_contigs, uint8_t *__restrict__ flag) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint64_t cs = cstart[walk_contig_of(cstart, n_contigs, pos[j])];
	const bool has1 = j >= 1 && pos[j - 1] >= cs, has2 = j >= 2 && pos[j - 2] >= cs;
	const uint32_t prev = has1 ? keys[j - 1] : 111111u;        // PrefixTable.cpp:335-336: lastPrefix starts as 111111 per contig
	bool store = true;
	if (keys[j] == prev) {
		// the bin remembered when k-mer j is looked at: none after a k-mer that differed from ITS predecessor
		bool have_bin = false;
		if (has1) { const uint32_t prev2 = has2 ? keys[j - 2] : 111111u; have_bin = keys[j - 1] == prev2; }
		if (have_bin && (pos[j] >> bin_shift) == (pos[j - 1] >> bin_shift)) store = false;
	}
	flag[j] = store ? 1 : 0;
}

// -> d_keys / d_vals (device, n entries, genome order).  Returns 0 or a negative error.
// carried walk state (CompactPrefixTable::lastPrefix / lastBin) after the last contig, and the visited k-mer count: --vcf needs both
struct WalkEnd { uint64_t visited = 0; uint32_t last_prefix = 111111u; int64_t last_bin = -1; };

int gpu_kmer_walk(ngm_ref *r, Buf<uint32_t> &keys_out, Buf<uint32_t> &vals_out, uint64_t *n_out, WalkEnd *end) {
	const uint64_t n = r->n_bases;
	const int k = r->prm.kmer, nc = (int) r->contigs.size();
	std::vector<uint64_t> hs(nc), he(nc);
	for (int c = 0; c < nc; ++c) { hs[c] = r->contigs[c].start; he[c] = r->contigs[c].start + r->contigs[c].len; }
	// (every return frees what the walk still holds: up to ~12 GB of scratch for a human-size genome)
	Buf<uint64_t> d_cs, d_ce, d_count;
	Buf<uint32_t> d_run, d_pos, d_keys, d_keys2, d_pos2;
	Buf<uint8_t> d_flag, d_tmp;
	NGM_MEM_TRY(d_cs.alloc(std::max(1, nc))); NGM_MEM_TRY(d_ce.alloc(std::max(1, nc)));
	REF_HIP_TRY(hipMemcpy(d_cs.p, hs.data(), nc * 8, hipMemcpyHostToDevice)); REF_HIP_TRY(hipMemcpy(d_ce.p, he.data(), nc * 8, hipMemcpyHostToDevice));
	NGM_MEM_TRY(d_run.alloc(std::max<uint64_t>(n, 1))); NGM_MEM_TRY(d_flag.alloc(std::max<uint64_t>(n, 1))); NGM_MEM_TRY(d_count.alloc(1));
	const unsigned nb = (unsigned) ((n + 255) / 256);
	hipLaunchKernelGGL(walk_mark_n_kernel, dim3(nb), dim3(256), 0, 0, r->d_genome.p, n, d_run.p);
	if (nc > 0) hipLaunchKernelGGL(walk_unmark_tails_kernel, dim3((nc + 255) / 256), dim3(256), 0, 0, d_ce.p, nc, d_run.p);
	size_t tb = 0, tb2 = 0;
	(void) rocprim::inclusive_scan(nullptr, tb, d_run.p, d_run.p, (size_t) n, rocprim::maximum<uint32_t>());
	(void) rocprim::select(nullptr, tb2, rocprim::counting_iterator<uint32_t>(0), d_flag.p, (uint32_t *) nullptr, d_count.p, (size_t) n);
	size_t tb3 = 0;
	(void) rocprim::select(nullptr, tb3, (uint32_t *) nullptr, d_flag.p, (uint32_t *) nullptr, d_count.p, (size_t) n);
	tb = std::max(tb, std::max(tb2, tb3)) + 256;
	NGM_MEM_TRY(d_tmp.alloc(tb));
	REF_HIP_TRY(rocprim::inclusive_scan(d_tmp.p, tb, d_run.p, d_run.p, (size_t) n, rocprim::maximum<uint32_t>()));
	hipLaunchKernelGGL(walk_visit_flags_kernel, dim3(nb), dim3(256), 0, 0, d_run.p, r->d_genome.p, n, k, r->prm.kmer_skip + 1, d_cs.p, d_ce.p, nc, d_flag.p);
	REF_HIP_TRY(hipGetLastError());
	// upper bound of visited k-mers: every (skip+1)-th position plus one per run
	const uint64_t cap = n / (uint64_t) (r->prm.kmer_skip + 1) + n / 1000 + 4096;
	NGM_MEM_TRY(d_pos.alloc(cap));
	REF_HIP_TRY(rocprim::select(d_tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), d_flag.p, d_pos.p, d_count.p, (size_t) n));
	uint64_t m = 0;
	REF_HIP_TRY(hipMemcpy(&m, d_count.p, 8, hipMemcpyDeviceToHost));
	if (m > cap) { ngm::pipeline_set_error("k-mer walk: more visited k-mers than expected"); return -75; }
	d_run.release();   // (early: its four bytes per base make room for the three arrays below)
	NGM_MEM_TRY(d_keys.alloc(std::max<uint64_t>(m, 1))); NGM_MEM_TRY(d_keys2.alloc(std::max<uint64_t>(m, 1))); NGM_MEM_TRY(d_pos2.alloc(std::max<uint64_t>(m, 1)));
	uint64_t kept = 0;
	if (m > 0) {
		const unsigned mb = (unsigned) ((m + 255) / 256);
		hipLaunchKernelGGL(walk_keys_kernel, dim3(mb), dim3(256), 0, 0, d_pos.p, m, r->d_genome.p, k, d_cs.p, d_ce.p, nc, d_keys.p);
		hipLaunchKernelGGL(walk_store_flags_kernel, dim3(mb), dim3(256), 0, 0, d_pos.p, d_keys.p, m, r->prm.bin_size, d_cs.p, nc, d_flag.p);
		REF_HIP_TRY(hipGetLastError());
		REF_HIP_TRY(rocprim::select(d_tmp.p, tb, d_keys.p, d_flag.p, d_keys2.p, d_count.p, (size_t) m));
		REF_HIP_TRY(rocprim::select(d_tmp.p, tb, d_pos.p, d_flag.p, d_pos2.p, d_count.p, (size_t) m));
		REF_HIP_TRY(hipMemcpy(&kept, d_count.p, 8, hipMemcpyDeviceToHost));
		if (end && nc > 0) {  // the state the last contig's walk leaves behind: from its last two visited k-mers
			uint32_t lk[2] = {0, 0}, lp[2] = {0, 0};
			const uint64_t t = m >= 2 ? m - 2 : 0, cnt = m - t;
			REF_HIP_TRY(hipMemcpy(lk, d_keys.p + t, cnt * 4, hipMemcpyDeviceToHost));
			REF_HIP_TRY(hipMemcpy(lp, d_pos.p + t, cnt * 4, hipMemcpyDeviceToHost));
			const uint64_t last_start = hs[nc - 1];
			const int in_last = (cnt >= 1 && lp[cnt - 1] >= last_start) + (cnt >= 2 && lp[0] >= last_start);
			if (in_last >= 1) {
				const uint32_t k1 = lk[cnt - 1], k0 = in_last == 2 ? lk[0] : 111111u;
				end->last_prefix = k1;
				end->last_bin = k1 == k0 ? (int64_t) (lp[cnt - 1] >> r->prm.bin_size) : -1;
			}
		}
	}
	if (end) end->visited = m;
	keys_out = std::move(d_keys2); vals_out = std::move(d_pos2); *n_out = kept;
	return 0;
}


// ---- --vcf: the k-mers of known variants (PrefixTable.cpp:500-574 BuildSNPTable, counted at :360-374, filled at :411-422) -------
// Every kept variant gives a region: the reference around it with the ALT spliced in, walked like a contig at positions
// ref_offset + i.  The count pass resets the walk state per region, the fill pass does not (its state comes from the last contig
// and from the region before): a k-mer list gets the count pass's number of slots, the fill pass's entries first (genome order,
// then VCF order) and zeros in the rest.  The first contig starts at 1000 and a region reaches at most k + |REF| + |ALT| - 2 bases
// to the left, which build_vcf_entries checks (the reference's unsigned underflow is not restated).
enum : uint8_t { kVarIgnored = 0, kVarSnp = 1, kVarIndel = 2, kVarBad = 3 };
constexpr uint32_t kVarX = 8;  // DecodeRefSequence's 'x' filler (never equal to a VCF base; encode('x') == 0 in the walk)

__host__ __device__ __forceinline__ uint32_t vcf_class_of(char c) {
	return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 5u;  // (the reader keeps ACGTN only)
}
// DecodeRefSequence(buffer, 0, off, region_len) (SequenceProvider.cpp:382-441): region_len - 2 bases from off, a last odd one and
// everything past the concatenated genome's end read as 'x'; an odd offset brings one base more
struct VcfGeom {
	uint64_t off; uint32_t d, dlen, b; bool x_last;
	__device__ VcfGeom(uint64_t pos, uint32_t half, uint64_t concat) {
		off = pos - half;
		uint64_t len = 2ull * half - 2, end = 0;
		if (off + len > concat) { end = off + len - concat; len -= end; }
		d = (uint32_t) ((off & 1) + 2 * ((len + 1) / 2));
		x_last = (len & 1) != 0;
		dlen = d + (uint32_t) end;
		b = half - 1;  // buffer_snp_pos
	}
	__device__ uint32_t cls(const uint32_t *g, uint32_t t) const { return (t >= d || (x_last && t == d - 1)) ? kVarX : d_class_at(g, off + t); }
};
__device__ __forceinline__ uint32_t vcf_half(const NgmVariant &v, int k) { return (uint32_t) k + v.ref_len + v.alt_len - 2; }

// one thread per variant: what BuildSNPTable does with it, and the length of its region; the first indel whose REF does not match
// the genome ends the table (the `break` at PrefixTable.cpp:553-554)
__global__ void vcf_classify_kernel(const NgmVariant *__restrict__ var, uint64_t n, const char *__restrict__ seq, const uint32_t *__restrict__ genome,
		uint64_t concat, int k, uint8_t *__restrict__ status, uint64_t *__restrict__ len, unsigned long long *__restrict__ first_bad) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const NgmVariant v = var[i];
	const VcfGeom g(v.pos, vcf_half(v, k), concat);
	uint8_t st;
	uint64_t l = 0;
	if (v.ref_len == 1 && v.alt_len == 1) {  // a SNP's REF is never looked at
		st = g.cls(genome, g.b) == vcf_class_of(seq[v.alt_off]) ? kVarIgnored : kVarSnp;
		if (st == kVarSnp) l = g.dlen;
	} else {
		st = (uint64_t) g.b + v.ref_len <= g.dlen ? kVarIndel : kVarBad;
		for (uint32_t t = 0; t < v.ref_len && st == kVarIndel; ++t)
			if (g.cls(genome, g.b + t) != vcf_class_of(seq[v.ref_off + t])) st = kVarBad;
		if (st == kVarIndel) l = (uint64_t) g.dlen - v.ref_len + v.alt_len;
		else atomicMin(first_bad, (unsigned long long) i);
	}
	status[i] = st;
	len[i] = l;
}
// regions after the first bad indel are dropped; counts for `Built SNP region table`: SNPs, indels, ignored
__global__ void vcf_cut_kernel(uint64_t n, const unsigned long long *__restrict__ first_bad, const uint8_t *__restrict__ status, uint64_t *__restrict__ len,
		unsigned long long *__restrict__ counts) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (i >= *first_bad) { len[i] = 0; return; }
	atomicAdd(&counts[status[i] == kVarSnp ? 0 : status[i] == kVarIndel ? 1 : 2], 1ull);
}
// region bytes (classes, 'x' as A) at the exclusive scan of the lengths
__global__ void vcf_fill_kernel(const NgmVariant *__restrict__ var, uint64_t n, const char *__restrict__ seq, const uint32_t *__restrict__ genome,
		uint64_t concat, int k, const uint64_t *__restrict__ len, const uint64_t *__restrict__ roff, uint8_t *__restrict__ out) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || len[i] == 0) return;
	const NgmVariant v = var[i];
	const VcfGeom g(v.pos, vcf_half(v, k), concat);
	uint8_t *o = out + roff[i];
	auto put = [&](uint32_t c) { *o++ = (uint8_t) (c == kVarX ? 0u : c); };
	if (v.ref_len == 1 && v.alt_len == 1) {
		for (uint32_t t = 0; t < g.dlen; ++t) put(t == g.b ? vcf_class_of(seq[v.alt_off]) : g.cls(genome, t));
	} else {
		for (uint32_t t = 0; t < g.b; ++t) put(g.cls(genome, t));
		for (uint32_t t = 0; t < v.alt_len; ++t) put(vcf_class_of(seq[v.alt_off + t]));
		for (uint32_t t = g.b + v.ref_len; t < g.dlen; ++t) put(g.cls(genome, t));
	}
}

// CS::PrefixIteration (CSstatic.cpp:26-76) over one region, calling f(prefix, position) for every VISITED k-mer -- KmerWalker::iterate
// without the store rule, for the host and the device
template <class F>
__host__ __device__ inline void vcf_walk_region(const uint8_t *seq, uint64_t length, uint64_t offset, int k, int skip, uint32_t mask, F &f) {
	for (;;) {
		if (length < (uint64_t) k) return;
		if (seq[0] == 5) {
			uint64_t n_skip = 1;
			while (n_skip < length && seq[n_skip] == 5) ++n_skip;
			seq += n_skip;
			if (n_skip >= (length - k)) return;  // CSstatic.cpp:37
			length -= n_skip;
			offset += n_skip;
		}
		uint32_t prefix = 0;
		bool restart = false;
		for (uint64_t i = 0; i < (uint64_t) k - 1; ++i) {
			if (seq[i] == 5) { seq += i + 1; length -= i + 1; offset += i + 1; restart = true; break; }
			prefix = (prefix << 2) | (seq[i] == 2 ? 3u : seq[i] == 3 ? 2u : (uint32_t) seq[i]);
		}
		if (restart) continue;
		int skipcount = skip;
		for (uint64_t i = k - 1; i < length; ++i) {
			if (seq[i] == 5) { seq += i + 1; length -= i + 1; offset += i + 1; restart = true; break; }
			prefix = ((prefix << 2) | (seq[i] == 2 ? 3u : seq[i] == 3 ? 2u : (uint32_t) seq[i])) & mask;
			if (skipcount == skip) { f(prefix, offset + i + 1 - k); skipcount = 0; }
			else ++skipcount;
		}
		if (!restart) return;
	}
}
// one thread per region: the number of visited k-mers (WRITE = false), or the k-mers themselves at their offset
template <bool WRITE>
__global__ void vcf_walk_kernel(const NgmVariant *__restrict__ var, uint64_t n, int k, int skip, const uint64_t *__restrict__ len,
		const uint64_t *__restrict__ roff, const uint8_t *__restrict__ regions, uint64_t *__restrict__ vcount, const uint64_t *__restrict__ voff,
		uint32_t *__restrict__ keys, uint32_t *__restrict__ pos, uint32_t *__restrict__ reg) {
	const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (len[i] == 0) { if (!WRITE) vcount[i] = 0; return; }
	const NgmVariant v = var[i];
	const uint64_t off = v.pos - vcf_half(v, k);
	const uint32_t mask = (1u << (2 * k)) - 1u;
	if (!WRITE) {
		uint64_t c = 0;
		auto f = [&](uint32_t, uint64_t) { ++c; };
		vcf_walk_region(regions + roff[i], len[i], off, k, skip, mask, f);
		vcount[i] = c;
	} else {
		uint64_t o = voff[i];
		auto f = [&](uint32_t p, uint64_t q) { keys[o] = p; pos[o] = (uint32_t) q; reg[o] = (uint32_t) i; ++o; };
		vcf_walk_region(regions + roff[i], len[i], off, k, skip, mask, f);
	}
}
// the store rule (CountKmer / BuildPrefixTable, PrefixTable.cpp:641-709) of visited region k-mer j under both passes: the state before
// j follows from the two visited k-mers before it -- within its region for the count flag (bit 0), across regions and from the
// genome's end state (cp, cb) for the fill flag (bit 1)
__global__ void vcf_store_flags_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ reg, uint64_t m,
		int bin_shift, uint32_t cp, long long cb, uint8_t *__restrict__ cflag, uint8_t *__restrict__ fflag) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const long long bin = (long long) (pos[j] >> bin_shift);
	auto store = [&](uint32_t lp, long long lb) { return keys[j] != lp || lb == -1 || bin != lb; };
	const bool first = j == 0 || reg[j - 1] != reg[j];
	{
		uint32_t lp = 111111u; long long lb = -1;
		if (!first) {
			lp = keys[j - 1];
			const bool first1 = j - 1 == 0 || reg[j - 2] != reg[j - 1];
			lb = keys[j - 1] == (first1 ? 111111u : keys[j - 2]) ? (long long) (pos[j - 1] >> bin_shift) : -1;
		}
		cflag[j] = store(lp, lb) ? 1 : 0;
	}
	{
		uint32_t lp = cp; long long lb = cb;
		if (j > 0) {
			lp = keys[j - 1];
			lb = keys[j - 1] == (j - 1 == 0 ? cp : keys[j - 2]) ? (long long) (pos[j - 1] >> bin_shift) : -1;
		}
		fflag[j] = store(lp, lb) ? 1 : 0;
	}
}
// merge: count-pass entries add slots, fill-pass entries (already in the sorted table) take theirs back
__global__ void vcf_slot_delta_kernel(const uint32_t *__restrict__ keys, uint64_t n, int delta, uint32_t *__restrict__ raw) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n) atomicAdd(&raw[keys[j]], (uint32_t) delta);
}
// sorted entry j of k-mer kj goes to the kj's new list at its rank; the slots behind the fill pass's entries stay 0
__global__ void vcf_scatter_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t n, const uint2 *__restrict__ old_index,
		const uint32_t *__restrict__ start, const uint32_t *__restrict__ raw, uint32_t *__restrict__ out, unsigned int *__restrict__ overflow) {
	const uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n) return;
	const uint32_t kj = keys[j], rank = (uint32_t) j - old_index[kj].x;
	if (rank < raw[kj]) out[(uint64_t) start[kj] + rank] = vals[j];
	else atomicAdd(overflow, 1u);
}
__global__ void vcf_narrow_kernel(uint32_t n_kmers, const uint64_t *__restrict__ start64, uint32_t *__restrict__ start) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p < n_kmers) start[p] = (uint32_t) start64[p];
}
__global__ void vcf_index_kernel(uint32_t n_kmers, const uint32_t *__restrict__ start, const uint32_t *__restrict__ raw, uint2 *__restrict__ index) {
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p < n_kmers) index[p] = make_uint2(start[p], raw[p]);
}

// what the variants add to the table: fill-pass entries (keys + positions, VCF order) and count-pass keys
struct VcfEntries {
	Buf<uint32_t> d_fkeys, d_fvals, d_ckeys;
	uint64_t nf = 0, nc = 0, visited = 0;
};

// regions on the GPU; their walk on the GPU, or (host_walk) on the host like KmerWalker
int build_vcf_entries(ngm_ref *r, const WalkEnd &end, bool host_walk, VcfEntries &out) {
	const NgmVcf &vcf = *r->vcf;
	const int k = r->prm.kmer;
	const uint64_t n = vcf.v.size(), concat = r->n_bases - 1;
	r->vcf_summary[0] = n;
	if (n == 0) return 0;
	for (const NgmVariant &v : vcf.v) {
		const uint64_t half = (uint64_t) k + v.ref_len + v.alt_len - 2;
		if (v.pos < half) { ngm::pipeline_set_error("VCF variant at %llu: its region would start before the genome", (unsigned long long) v.pos); return -22; }
		if (v.pos - half >= concat) { ngm::pipeline_set_error("VCF variant at %llu lies beyond the end of the genome", (unsigned long long) v.pos); return -22; }
	}
	Buf<NgmVariant> d_var;
	Buf<char> d_seq;
	Buf<uint8_t> d_status, d_regions, d_cf, d_ff, d_tmp;
	Buf<uint64_t> d_len, d_roff, d_vcount, d_voff, d_sel;
	Buf<unsigned long long> d_bad, d_counts;
	Buf<uint32_t> d_vk, d_vp, d_vr;
	NGM_MEM_TRY(d_var.alloc(n));
	NGM_MEM_TRY(d_seq.alloc(std::max<size_t>(vcf.seq.size(), 1)));
	REF_HIP_TRY(hipMemcpy(d_var.p, vcf.v.data(), n * sizeof(NgmVariant), hipMemcpyHostToDevice));
	REF_HIP_TRY(hipMemcpy(d_seq.p, vcf.seq.data(), vcf.seq.size(), hipMemcpyHostToDevice));
	NGM_MEM_TRY(d_status.alloc(n)); NGM_MEM_TRY(d_len.alloc(n)); NGM_MEM_TRY(d_roff.alloc(n));
	NGM_MEM_TRY(d_bad.alloc(1)); NGM_MEM_TRY(d_counts.alloc(3)); NGM_MEM_TRY(d_sel.alloc(1));
	const unsigned long long none = ~0ull;
	REF_HIP_TRY(hipMemcpy(d_bad.p, &none, 8, hipMemcpyHostToDevice));
	REF_HIP_TRY(hipMemset(d_counts.p, 0, 3 * 8));
	const unsigned nb = (unsigned) ((n + 255) / 256);
	hipLaunchKernelGGL(vcf_classify_kernel, dim3(nb), dim3(256), 0, 0, d_var.p, n, d_seq.p, r->d_genome.p, concat, k, d_status.p, d_len.p, d_bad.p);
	hipLaunchKernelGGL(vcf_cut_kernel, dim3(nb), dim3(256), 0, 0, n, d_bad.p, d_status.p, d_len.p, d_counts.p);
	REF_HIP_TRY(hipGetLastError());
	unsigned long long counts[3], bad = 0;
	REF_HIP_TRY(hipMemcpy(counts, d_counts.p, 3 * 8, hipMemcpyDeviceToHost));
	REF_HIP_TRY(hipMemcpy(&bad, d_bad.p, 8, hipMemcpyDeviceToHost));
	if (bad != none) fprintf(stderr, "[PREPROCESS] SNP ref does not match reference at SNP %llu\n", (unsigned long long) vcf.v[bad].pos);
	r->vcf_summary[1] = counts[0]; r->vcf_summary[2] = counts[1]; r->vcf_summary[3] = counts[2] + (bad != none ? 1 : 0);
	size_t tb = 0;
	REF_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, d_len.p, d_roff.p, (uint64_t) 0, (size_t) n, rocprim::plus<uint64_t>()));
	tb += 256;
	NGM_MEM_TRY(d_tmp.alloc(tb));
	REF_HIP_TRY(rocprim::exclusive_scan(d_tmp.p, tb, d_len.p, d_roff.p, (uint64_t) 0, (size_t) n, rocprim::plus<uint64_t>()));
	uint64_t last_off = 0, last_len = 0;
	REF_HIP_TRY(hipMemcpy(&last_off, d_roff.p + n - 1, 8, hipMemcpyDeviceToHost));
	REF_HIP_TRY(hipMemcpy(&last_len, d_len.p + n - 1, 8, hipMemcpyDeviceToHost));
	const uint64_t total = last_off + last_len;
	NGM_MEM_TRY(d_regions.alloc(std::max<uint64_t>(total, 1)));
	hipLaunchKernelGGL(vcf_fill_kernel, dim3(nb), dim3(256), 0, 0, d_var.p, n, d_seq.p, r->d_genome.p, concat, k, d_len.p, d_roff.p, d_regions.p);
	REF_HIP_TRY(hipGetLastError());
	const uint32_t mask = (1u << (2 * k)) - 1u;
	const int bin_shift = r->prm.bin_size, skip = r->prm.kmer_skip;
	if (host_walk) {
		// the two walkers of the reference: the count pass restarts its state per region, the fill pass carries it on
		std::vector<uint8_t> reg(total);
		std::vector<uint64_t> len(n), roff(n);
		REF_HIP_TRY(hipMemcpy(reg.data(), d_regions.p, total, hipMemcpyDeviceToHost));
		REF_HIP_TRY(hipMemcpy(len.data(), d_len.p, n * 8, hipMemcpyDeviceToHost));
		REF_HIP_TRY(hipMemcpy(roff.data(), d_roff.p, n * 8, hipMemcpyDeviceToHost));
		std::vector<uint32_t> fk, fv, ck;
		uint32_t fp = end.last_prefix, cpfx = 111111u;
		int64_t fb = end.last_bin, cbin = -1;
		uint64_t visited = 0;
		auto f = [&](uint32_t prefix, uint64_t pos) {
			const int64_t bin = (int64_t) (pos >> bin_shift);
			++visited;
			auto step = [&](uint32_t &lp, int64_t &lb) {
				bool st = true;
				if (prefix == lp) { if (!(bin != lb || lb == -1)) st = false; lb = bin; }
				else lb = -1;
				lp = prefix;
				return st;
			};
			if (step(cpfx, cbin)) ck.push_back(prefix);
			if (step(fp, fb)) { fk.push_back(prefix); fv.push_back((uint32_t) pos); }
		};
		for (uint64_t i = 0; i < n; ++i) {
			if (!len[i]) continue;
			cpfx = 111111u; cbin = -1;
			const NgmVariant &v = vcf.v[i];
			vcf_walk_region(reg.data() + roff[i], len[i], v.pos - ((uint64_t) k + v.ref_len + v.alt_len - 2), k, skip, mask, f);
		}
		out.visited = visited; out.nf = fk.size(); out.nc = ck.size();
		NGM_MEM_TRY(out.d_fkeys.alloc(std::max<uint64_t>(out.nf, 1))); NGM_MEM_TRY(out.d_fvals.alloc(std::max<uint64_t>(out.nf, 1)));
		NGM_MEM_TRY(out.d_ckeys.alloc(std::max<uint64_t>(out.nc, 1)));
		REF_HIP_TRY(hipMemcpy(out.d_fkeys.p, fk.data(), out.nf * 4, hipMemcpyHostToDevice));
		REF_HIP_TRY(hipMemcpy(out.d_fvals.p, fv.data(), out.nf * 4, hipMemcpyHostToDevice));
		REF_HIP_TRY(hipMemcpy(out.d_ckeys.p, ck.data(), out.nc * 4, hipMemcpyHostToDevice));
		return 0;
	}
	NGM_MEM_TRY(d_vcount.alloc(n)); NGM_MEM_TRY(d_voff.alloc(n));
	hipLaunchKernelGGL(vcf_walk_kernel<false>, dim3(nb), dim3(256), 0, 0, d_var.p, n, k, skip, d_len.p, d_roff.p, d_regions.p, d_vcount.p, nullptr, nullptr, nullptr, nullptr);
	REF_HIP_TRY(hipGetLastError());
	REF_HIP_TRY(rocprim::exclusive_scan(d_tmp.p, tb, d_vcount.p, d_voff.p, (uint64_t) 0, (size_t) n, rocprim::plus<uint64_t>()));
	REF_HIP_TRY(hipMemcpy(&last_off, d_voff.p + n - 1, 8, hipMemcpyDeviceToHost));
	REF_HIP_TRY(hipMemcpy(&last_len, d_vcount.p + n - 1, 8, hipMemcpyDeviceToHost));
	const uint64_t m = last_off + last_len;
	out.visited = m;
	if (m == 0) return 0;
	NGM_MEM_TRY(d_vk.alloc(m)); NGM_MEM_TRY(d_vp.alloc(m)); NGM_MEM_TRY(d_vr.alloc(m));
	hipLaunchKernelGGL(vcf_walk_kernel<true>, dim3(nb), dim3(256), 0, 0, d_var.p, n, k, skip, d_len.p, d_roff.p, d_regions.p, nullptr, d_voff.p, d_vk.p, d_vp.p, d_vr.p);
	NGM_MEM_TRY(d_cf.alloc(m)); NGM_MEM_TRY(d_ff.alloc(m));
	const unsigned mb = (unsigned) ((m + 255) / 256);
	hipLaunchKernelGGL(vcf_store_flags_kernel, dim3(mb), dim3(256), 0, 0, d_vk.p, d_vp.p, d_vr.p, m, bin_shift, end.last_prefix, (long long) end.last_bin, d_cf.p, d_ff.p);
	REF_HIP_TRY(hipGetLastError());
	d_tmp.release();   // (early: the select's storage is sized anew)
	tb = 0;
	REF_HIP_TRY(rocprim::select(nullptr, tb, d_vk.p, d_ff.p, (uint32_t *) nullptr, d_sel.p, (size_t) m));
	tb += 256;
	NGM_MEM_TRY(d_tmp.alloc(tb));
	NGM_MEM_TRY(out.d_fkeys.alloc(m)); NGM_MEM_TRY(out.d_fvals.alloc(m)); NGM_MEM_TRY(out.d_ckeys.alloc(m));
	REF_HIP_TRY(rocprim::select(d_tmp.p, tb, d_vk.p, d_ff.p, out.d_fkeys.p, d_sel.p, (size_t) m));
	REF_HIP_TRY(rocprim::select(d_tmp.p, tb, d_vp.p, d_ff.p, out.d_fvals.p, d_sel.p, (size_t) m));
	REF_HIP_TRY(hipMemcpy(&out.nf, d_sel.p, 8, hipMemcpyDeviceToHost));
	REF_HIP_TRY(rocprim::select(d_tmp.p, tb, d_vk.p, d_cf.p, out.d_ckeys.p, d_sel.p, (size_t) m));
	REF_HIP_TRY(hipMemcpy(&out.nc, d_sel.p, 8, hipMemcpyDeviceToHost));
	return 0;
}

// bucket of k-mer p: word 0 = own list length (bits 0-13; 0: unused, or more than 9900 occurrences) | list length of the
// reverse-complement k-mer << 14 (the search needs the sum of both, CS.cpp:122) | 1 << 31 when the list does not fit;
// words 1.. = the positions, or word 1 = start in d_positions for a list that does not fit.  One bucket more than there
// are k-mers: the last one stays zero (what lanes without a list read).  One thread per bucket word: coalesced stores.
__global__ void fill_buckets_kernel(uint32_t n_kmers, int k, int log2_w, const uint2 *__restrict__ index, const uint32_t *__restrict__ positions,
		uint32_t *__restrict__ buckets) {
	const uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t p = (uint32_t) (g >> log2_w), w = (uint32_t) g & ((1u << log2_w) - 1u);
	if (p > n_kmers) return;
	if (p == n_kmers) { buckets[g] = 0; return; }
	const uint2 e = index[p];
	const bool inl = e.y < (1u << log2_w);
	uint32_t v = 0;
	if (w == 0) v = e.y | (index[d_revcomp(p, k)].y << 14) | (inl ? 0u : 0x80000000u);
	else if (inl) v = (w <= e.y) ? positions[e.x + (w - 1)] : 0u;
	else if (w == 1) v = e.x;
	buckets[g] = v;
}

// canonical bucket c (refindex.h): the pair {X = kmer_of_canon_id(c), revcomp(X)}
__global__ void fill_cbuckets_kernel(uint32_t n_pairs, int k, int log2_w, const uint2 *__restrict__ index, const uint32_t *__restrict__ positions,
		uint32_t *__restrict__ buckets) {
	const uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t c = (uint32_t) (g >> log2_w), w = (uint32_t) g & ((1u << log2_w) - 1u);
	if (c >= n_pairs) return;
	const int b = 2 * (k / 2) + 1;
	const uint32_t x = ((c >> b) << (b + 1)) | (c & ((1u << b) - 1u));
	const uint2 ea = index[x], eb = index[d_revcomp(x, k)];
	const uint32_t na = ea.y, nb = eb.y;
	const bool inl = na + nb < (1u << log2_w);
	uint32_t v = 0;
	if (w == 0) v = na | (nb << 14) | (inl ? 0u : 0x80000000u);
	else if (inl) v = (w <= na) ? positions[ea.x + (w - 1)] : (w <= na + nb) ? positions[eb.x + (w - 1 - na)] : 0u;
	else if (w == 1) v = ea.x;
	else if (w == 2) v = eb.x;
	buckets[g] = v;
}

std::mutex g_bucket_mu;

int build_buckets_kind(ngm_ref *r, int kind) {
	const int k = r->prm.kmer;
	const uint32_t n_kmers = 1u << (2 * k);
	if (kind == 1) {
		if (r->d_cbuckets.p) return 0;
		if ((k & 1) == 0) { ngm::pipeline_set_error("canonical buckets need an odd k-mer length"); return -22; }
		const uint32_t n_pairs = n_kmers / 2;
		const double mu = (double) r->n_entries / (double) n_pairs;
		int lw = 2;
		while (lw < 6 && (double) ((1 << lw) - 1) < mu + 4.0 * sqrt(mu) + 0.5) ++lw;
		while (lw > 2 && ((uint64_t) n_pairs << lw) + r->n_entries + 16 >= 0xFFFFFFFFull) --lw;
		const uint64_t words = (uint64_t) n_pairs << lw;
		Buf<uint32_t> d;
		NGM_MEM_TRY(d.alloc(words + r->n_entries + 16));
		hipLaunchKernelGGL(fill_cbuckets_kernel, dim3((unsigned) ((words + 255) / 256)), dim3(256), 0, 0, n_pairs, k, lw, r->d_index.p, r->d_positions.p, d.p);
		if (hipGetLastError() != hipSuccess || hipMemcpy(d.p + words, r->d_positions.p, (r->n_entries + 16) * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
				hipDeviceSynchronize() != hipSuccess) { ngm::pipeline_set_error("building the canonical buckets failed"); return -5; }
		r->cbucket_log2_words = lw;
		r->cbucket_pos_base = (uint32_t) words;
		r->d_cbuckets = std::move(d);
		return 0;
	}
	if (r->d_buckets.p) return 0;
	// W - 1 >= mean + 4 standard deviations of a Poisson list length (real genomes have a heavy tail on top: those
	// lists overflow into d_positions, which costs them one more request)
	const double mu = (double) r->n_entries / (double) n_kmers;
	int lw = 2;
	while (lw < 5 && (double) ((1 << lw) - 1) < mu + 4.0 * sqrt(mu) + 0.5) ++lw;
	// the buckets are followed by a copy of the position table, so that one 32-bit word offset addresses an inline list and a
	// list that did not fit alike; both must stay below 2^32 words
	while (lw > 2 && (((uint64_t) n_kmers + 1) << lw) + r->n_entries + 16 >= 0xFFFFFFFFull) --lw;
	const uint64_t words = ((uint64_t) n_kmers + 1) << lw;
	Buf<uint32_t> d;
	NGM_MEM_TRY(d.alloc(words + r->n_entries + 16));
	hipLaunchKernelGGL(fill_buckets_kernel, dim3((unsigned) ((words + 255) / 256)), dim3(256), 0, 0, n_kmers, k, lw, r->d_index.p, r->d_positions.p, d.p);
	if (hipGetLastError() != hipSuccess || hipMemcpy(d.p + words, r->d_positions.p, (r->n_entries + 16) * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
			hipDeviceSynchronize() != hipSuccess) { ngm::pipeline_set_error("building the buckets failed"); return -5; }
	r->bucket_log2_words = lw;
	r->bucket_pos_base = (uint32_t) words;
	r->d_buckets = std::move(d);
	return 0;
}

int build_index(ngm_ref *r) {
	const int k = r->prm.kmer;
	const uint32_t n_kmers = 1u << (2 * k);
	Buf<uint32_t> d_keys, d_vals, d_keys2, d_starts;
	uint64_t n = 0;
	WalkEnd end;
	// NGM_HIP_TEST_LIMITS=host_walk=1: the host walk below, as taken when the GPU walk runs out of memory
	const bool host_walk = ngm::test_limit("host_walk", 0) != 0;
	if (!host_walk) {
		// the walk on the GPU (CountKmerFreq decodes a contig with bufferLength = len and DecodeRefSequence emits len - 2 bases,
		// 'x' / NUL after that, which encode() maps to 0: the last two bases of a contig act as 'A' -- handled in the kernels)
		if (gpu_kmer_walk(r, d_keys, d_vals, &n, &end) != 0) { n = 0; end = WalkEnd(); (void) hipGetLastError(); }  // e.g. out of memory on a shared GPU: the host walk needs no scratch
	}
	const bool walked_on_host = !d_keys.p;
	if (walked_on_host) {
		std::vector<uint32_t> keys, vals;
		keys.reserve(r->n_bases / (r->prm.kmer_skip + 1) + 16);
		vals.reserve(r->n_bases / (r->prm.kmer_skip + 1) + 16);
		KmerWalker w{k, r->prm.kmer_skip, r->prm.bin_size, (k == 16) ? 0xFFFFFFFFu : ((1u << (2 * k)) - 1u), 111111u, -1, &keys, &vals};
		std::vector<uint8_t> tmp;
		for (const NgmContig &c : r->contigs) {
			w.last_prefix = 111111u;  // PrefixTable.cpp:335-336
			w.last_bin = -1;
			// CountKmerFreq decodes the contig with bufferLength = len, and DecodeRefSequence emits bufferLength-2
			// bases ('x' / NUL after that, SequenceProvider.cpp:384, :424-439); PrefixIteration then still walks
			// all len characters and encode() maps both fillers to 0: the last two bases act as 'A'.
			tmp.assign(r->host_cls.begin() + c.start, r->host_cls.begin() + c.start + c.len);
			if (c.len >= 2) { tmp[c.len - 2] = 0; tmp[c.len - 1] = 0; }
			w.iterate(tmp.data(), c.len, c.start);
		}
		end.visited = w.visited; end.last_prefix = w.last_prefix; end.last_bin = w.last_bin;
		n = keys.size();
		NGM_MEM_TRY(d_keys.alloc(std::max<uint64_t>(n, 1)));
		NGM_MEM_TRY(d_vals.alloc(std::max<uint64_t>(n, 1)));
		REF_HIP_TRY(hipMemcpy(d_keys.p, keys.data(), n * 4, hipMemcpyHostToDevice));
		REF_HIP_TRY(hipMemcpy(d_vals.p, vals.data(), n * 4, hipMemcpyHostToDevice));
	}
	VcfEntries ve;
	if (r->vcf) {
		// the variants' fill-pass entries go behind the genome's, so the stable sort keeps each list in the reference's order
		if (int rc = build_vcf_entries(r, end, walked_on_host, ve)) return rc;
		Buf<uint32_t> k2, v2;
		if (k2.alloc(std::max<uint64_t>(n + ve.nf, 1)) || v2.alloc(std::max<uint64_t>(n + ve.nf, 1))) {
			ngm::pipeline_set_error("out of device memory adding the VCF's k-mers");
			return -12;
		}
		REF_HIP_TRY(hipMemcpy(k2.p, d_keys.p, n * 4, hipMemcpyDeviceToDevice)); REF_HIP_TRY(hipMemcpy(v2.p, d_vals.p, n * 4, hipMemcpyDeviceToDevice));
		REF_HIP_TRY(hipMemcpy(k2.p + n, ve.d_fkeys.p, ve.nf * 4, hipMemcpyDeviceToDevice)); REF_HIP_TRY(hipMemcpy(v2.p + n, ve.d_fvals.p, ve.nf * 4, hipMemcpyDeviceToDevice));
		d_keys = std::move(k2); d_vals = std::move(v2);   // (the genome's own lists go here)
		const uint64_t genome_skips = end.visited - n;
		r->vcf_skip_count = genome_skips + ve.visited - ve.nc;
		r->vcf_skip_build = genome_skips + ve.visited - ve.nf;
		r->vcf_summary[4] = ve.nf;
		r->vcf_summary[5] = ve.nc - ve.nf;
		r->vcf_applied = true;
		n += ve.nf;
	}
	r->n_entries = n;
	NGM_MEM_TRY(d_keys2.alloc(std::max<uint64_t>(n, 1)));
	NGM_MEM_TRY(r->d_positions.alloc(std::max<uint64_t>(n, 1) + 16));  // the search reads 16-entry segments
	REF_HIP_TRY(hipMemset(r->d_positions.p, 0, (std::max<uint64_t>(n, 1) + 16) * 4));
	NGM_MEM_TRY(d_starts.alloc(n_kmers));
	NGM_MEM_TRY(r->d_raw_counts.alloc(n_kmers));
	NGM_MEM_TRY(r->d_index.alloc(n_kmers));
	REF_HIP_TRY(hipMemset(d_starts.p, 0, (size_t) n_kmers * 4));
	REF_HIP_TRY(hipMemset(r->d_raw_counts.p, 0, (size_t) n_kmers * 4));
	if (n > 0) {
		// stable LSD radix sort on the 2k key bits: inside each k-mer group the entries keep their input order -- ascending genome
		// positions, which is the order BuildPrefixTable appends them in (PrefixTable.cpp:729-748), followed with --vcf by the
		// variant regions' entries in VCF order (not ascending, and a position may repeat: refindex.h)
		size_t tmp_bytes = 0;
		REF_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_keys.p, d_keys2.p, d_vals.p, r->d_positions.p, n, 0, 2 * k));
		Buf<uint8_t> d_tmp;
		NGM_MEM_TRY(d_tmp.alloc(tmp_bytes));
		REF_HIP_TRY(rocprim::radix_sort_pairs(d_tmp.p, tmp_bytes, d_keys.p, d_keys2.p, d_vals.p, r->d_positions.p, n, 0, 2 * k));
		hipLaunchKernelGGL(mark_runs_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, d_keys2.p, n, d_starts.p, r->d_raw_counts.p);
		REF_HIP_TRY(hipGetLastError());
		REF_HIP_TRY(hipDeviceSynchronize());
	}   // (the sort's storage goes here)
	hipLaunchKernelGGL(finish_index_kernel, dim3((n_kmers + 255) / 256), dim3(256), 0, 0, n_kmers, k, d_starts.p, r->d_raw_counts.p, r->d_index.p);
	if (r->vcf) {
		// every list gets the count pass's number of slots (PrefixTable.cpp:360-374): its entries so far, then zeros
		if (ve.nc) hipLaunchKernelGGL(vcf_slot_delta_kernel, dim3((unsigned) ((ve.nc + 255) / 256)), dim3(256), 0, 0, ve.d_ckeys.p, ve.nc, 1, r->d_raw_counts.p);
		if (ve.nf) hipLaunchKernelGGL(vcf_slot_delta_kernel, dim3((unsigned) ((ve.nf + 255) / 256)), dim3(256), 0, 0, ve.d_fkeys.p, ve.nf, -1, r->d_raw_counts.p);
		REF_HIP_TRY(hipGetLastError());
		// new list starts: exclusive scan of the new lengths (in 64 bits, so that a table beyond 2^32 entries is caught)
		uint64_t total = 0;
		{
			Buf<uint64_t> d_start64;
			Buf<uint8_t> d_scan;
			size_t sb = 0;
			auto widen = rocprim::make_transform_iterator(r->d_raw_counts.p, [] __host__ __device__ (uint32_t x) { return (uint64_t) x; });
			REF_HIP_TRY(rocprim::exclusive_scan(nullptr, sb, widen, d_start64.p, (uint64_t) 0, (size_t) n_kmers, rocprim::plus<uint64_t>()));
			NGM_MEM_TRY(d_start64.alloc(n_kmers));
			if (d_scan.alloc(sb + 256)) { ngm::pipeline_set_error("out of device memory (VCF list starts)"); return -12; }
			const hipError_t e1 = rocprim::exclusive_scan(d_scan.p, sb, widen, d_start64.p, (uint64_t) 0, (size_t) n_kmers, rocprim::plus<uint64_t>());
			uint64_t last_start = 0;
			uint32_t last_raw = 0;
			const hipError_t e2 = hipMemcpy(&last_start, d_start64.p + n_kmers - 1, 8, hipMemcpyDeviceToHost);
			const hipError_t e3 = hipMemcpy(&last_raw, r->d_raw_counts.p + n_kmers - 1, 4, hipMemcpyDeviceToHost);
			total = last_start + last_raw;
			if (e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess && total + 16 < 0xFFFFFFFFull)
				hipLaunchKernelGGL(vcf_narrow_kernel, dim3((n_kmers + 255) / 256), dim3(256), 0, 0, n_kmers, d_start64.p, d_starts.p);
			d_scan.release();
			const hipError_t e4 = hipDeviceSynchronize();
			d_start64.release();
			if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) { ngm::pipeline_set_error("scanning the VCF list lengths failed"); return -5; }
			if (total + 16 >= 0xFFFFFFFFull) { ngm::pipeline_set_error("k-mer table with the VCF's k-mers exceeds 2^32 entries"); return -27; }
		}
		Buf<uint32_t> d_final;
		Buf<unsigned int> d_over;
		NGM_MEM_TRY(d_final.alloc(total + 16));
		REF_HIP_TRY(hipMemset(d_final.p, 0, (total + 16) * 4));
		NGM_MEM_TRY(d_over.alloc(1));
		REF_HIP_TRY(hipMemset(d_over.p, 0, 4));
		if (n) hipLaunchKernelGGL(vcf_scatter_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, d_keys2.p, r->d_positions.p, n, r->d_index.p, d_starts.p, r->d_raw_counts.p, d_final.p, d_over.p);
		hipLaunchKernelGGL(vcf_index_kernel, dim3((n_kmers + 255) / 256), dim3(256), 0, 0, n_kmers, d_starts.p, r->d_raw_counts.p, r->d_index.p);
		REF_HIP_TRY(hipGetLastError());
		unsigned int over = 0;
		REF_HIP_TRY(hipMemcpy(&over, d_over.p, 4, hipMemcpyDeviceToHost));
		d_over.release();
		r->d_positions = std::move(d_final);   // (the table without the zero slots goes here)
		r->n_entries = n = total;
		// (the fill pass never stores more into a list than the count pass reserved: the two differ in the first two visited
		// k-mers of a region only, where the count pass stores and the fill pass may skip)
		if (over) { ngm::pipeline_set_error("VCF k-mers: the fill pass stored more entries than the count pass reserved (%u)", over); return -75; }
	}
	hipLaunchKernelGGL(apply_usage_rule_kernel, dim3((n_kmers + 255) / 256), dim3(256), 0, 0, n_kmers, k, r->d_raw_counts.p, r->d_index.p);
	REF_HIP_TRY(hipGetLastError());
	REF_HIP_TRY(hipDeviceSynchronize());
	d_keys.release(); d_vals.release(); d_keys2.release(); d_starts.release();   // (before the statistics' host array)

	std::vector<uint32_t> raw(n_kmers);
	REF_HIP_TRY(hipMemcpy(raw.data(), r->d_raw_counts.p, (size_t) n_kmers * 4, hipMemcpyDeviceToHost));
	index_stats(r, raw.data(), (uint32_t) raw.size());
	return 0;   // the bucket layouts are built when the first mapper asks for one (ngm_ref_ensure_buckets): a bisulfite run needs none
}

// CompactPrefixTable::stats (PrefixTable.cpp:150-194): integer sums are exact in double, order-free
void index_stats(ngm_ref *r, const uint32_t *raw, uint32_t n_kmers) {
	// (sums of integers below 2^53: exact in doubles whatever the order, so the pool threads may split them)
	std::mutex mu;
	double sum = 0.0, sum2 = 0.0;
	ngm::ThreadPool::instance().parallel_for((int) ((n_kmers + (1u << 18) - 1) >> 18), [&](int lo, int hi) {
		double s1 = 0.0, s2 = 0.0;
		for (uint32_t j = (uint32_t) lo << 18, e = (uint32_t) std::min<uint64_t>(n_kmers, (uint64_t) hi << 18); j < e; ++j) { s1 += raw[j]; s2 += (double) raw[j] * (double) raw[j]; }
		std::lock_guard<std::mutex> lk(mu);
		sum += s1; sum2 += s2;
	}, 1);
	const double len = (double) n_kmers;
	const double avg = sum / len;
	const double stdev = sqrt(sum2 / (len - 1) - 2.0 * avg * (sum / (len - 1)) + ((len * avg * avg) / (len - 1)));
	r->auto_max_kfreq = (int) ceil(std::max(100.0, avg + 5 * stdev));
}


// host -> device for the multi-GB arrays of the reference (pageable or file-mapped memory): the pool threads copy 32 MB pieces
// into two page-locked buffers, each piece travels while the next is copied
int upload_staged(void *dst, const void *src, size_t bytes) {
	constexpr size_t kPiece = (size_t) 32 << 20;
	if (bytes <= kPiece) { REF_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
	ngm::PinnedBuf<char> stage[2];
	hipEvent_t done[2] = {nullptr, nullptr};
	hipStream_t st = nullptr;
	int rc = 0;
	auto cleanup = [&] { for (hipEvent_t e : done) if (e) (void) hipEventDestroy(e); if (st) (void) hipStreamDestroy(st); };   // (the two buffers free themselves)
	if (stage[0].alloc(kPiece) || stage[1].alloc(kPiece) ||
			hipEventCreateWithFlags(&done[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&done[1], hipEventDisableTiming) != hipSuccess ||
			hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
		cleanup();
		stage[0].release(); stage[1].release();   // (early: the plain copy stages through page-locked memory of the runtime's own)
		REF_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));   // (no page-locked memory left: the plain copy)
		return 0;
	}
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	int turn = 0;
	for (size_t off = 0; off < bytes && rc == 0; off += kPiece, turn ^= 1) {
		const size_t nb = std::min(kPiece, bytes - off);
		if (off >= 2 * kPiece && hipEventSynchronize(done[turn]) != hipSuccess) { rc = -5; break; }
		const char *from = (const char *) src + off;
		char *to = stage[turn].p;
		const int parts = (int) ((nb + (1u << 20) - 1) >> 20);
		pool.parallel_for(parts, [&](int lo, int hi) { const size_t a = (size_t) lo << 20, b = std::min(nb, (size_t) hi << 20); memcpy(to + a, from + a, b - a); }, 1);
		if (hipMemcpyAsync((char *) dst + off, to, nb, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(done[turn], st) != hipSuccess) rc = -5;
	}
	if (hipStreamSynchronize(st) != hipSuccess) rc = -5;
	cleanup();
	if (rc) ngm::pipeline_set_error("copying the reference to the GPU failed");
	return rc;
}

int upload_genome(ngm_ref *r) {
	// artificial upper bound for positions on the last contig (SequenceProvider.cpp:378)
	r->start_pos.clear();
	for (const NgmContig &c : r->contigs) r->start_pos.push_back(c.start);
	if (!r->contigs.empty()) r->start_pos.push_back(r->contigs.back().start + r->contigs.back().len + 1000);
	// upload the genome as packed nibbles (+ one guard word so window reads never run off the end)
	r->genome_words = (r->n_bases + 7) / 8 + 64;
	std::vector<uint32_t, ngm::default_init_allocator<uint32_t>> packed(r->genome_words);
	{
		const uint64_t nb = r->n_bases, nw = (nb + 7) / 8;
		for (uint64_t wi = nw; wi < r->genome_words; ++wi) packed[wi] = 0x66666666u;  // NUL class beyond the end
		const uint8_t *cls = r->host_cls.data();
		uint32_t *out = packed.data();
		const int blocks = (int) ((nw + (1u << 17) - 1) >> 17);  // 128 Kword blocks on the pool threads
		ngm::ThreadPool::instance().parallel_for(blocks, [&](int lo, int hi) {
			for (uint64_t wi = (uint64_t) lo << 17, e = std::min<uint64_t>(nw, (uint64_t) hi << 17); wi < e; ++wi) {
				uint32_t w = 0x66666666u;
				for (int b = 0; b < 8; ++b) {
					const uint64_t i = wi * 8 + (uint64_t) b;
					if (i < nb) w = (w & ~(0xFu << (4 * b))) | ((uint32_t) cls[i] << (4 * b));
				}
				out[wi] = w;
			}
		}, 1);
	}
	NGM_MEM_TRY(r->d_genome.alloc(r->genome_words));
	return upload_staged(r->d_genome.p, packed.data(), r->genome_words * 4);
}

int finish_ref(ngm_ref *r) {
	if (int rc = upload_genome(r)) return rc;
	return build_index(r);
}

void append_spacer(ngm::ByteVec &g) { g.insert(g.end(), 1000, (uint8_t) 5); }

void append_contig(ngm_ref *r, const std::string &name, const uint8_t *seq, uint64_t len) {
	if (len <= 10) return;  // minRefSeqLen, SequenceProvider.h:71 / .cpp:300
	NgmContig c;
	c.name = name.substr(0, 100);
	c.start = r->host_cls.size();
	c.len = len;
	r->host_cls.reserve(r->host_cls.size() + len + 1002);
	r->host_cls.resize(c.start + len);
	{
		uint8_t *dst = r->host_cls.data() + c.start;
		const int blocks = (int) ((len + (1u << 20) - 1) >> 20);  // 1 Mbase blocks on the pool threads
		ngm::ThreadPool::instance().parallel_for(blocks, [&](int lo, int hi) {
			for (uint64_t i = (uint64_t) lo << 20, e = std::min<uint64_t>(len, (uint64_t) hi << 20); i < e; ++i) dst[i] = class_of_base(seq[i]);
		}, 1);
	}
	if (len & 1) r->host_cls.push_back(5);  // odd contig: the second nibble of the last byte is an N
	append_spacer(r->host_cls);
	r->contigs.push_back(c);
}

ngm_ref *new_ref(int device, const ngm_ref_params *p) {
	if (!p || p->kmer < 4 || p->kmer > 15 || p->kmer_skip < 0 || p->bin_size < 0 || p->bin_size > 8) {
		ngm::pipeline_set_error("ngm_ref_create: bad parameters (kmer 4..15, kmer_skip >= 0, bin_size 0..8)");
		return nullptr;
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		ngm::pipeline_set_error("ngm_ref_create: no HIP device available (this library has no CPU fallback)");
		return nullptr;
	}
	if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) {
		ngm::pipeline_set_error("ngm_ref_create: cannot select device %d", device);
		return nullptr;
	}
	ngm_ref *r = new ngm_ref();
	r->device = device;
	r->prm = *p;
	append_spacer(r->host_cls);  // padding so that windows never start at a negative position
	return r;
}

ngm_ref *seal(ngm_ref *r) {
	r->n_bases = r->host_cls.size();
	if (r->contigs.empty()) { ngm::pipeline_set_error("ngm_ref_create: no usable contig"); ngm_ref_destroy(r); return nullptr; }
	if (r->n_bases >= 0xFFFFFFFFull) { ngm::pipeline_set_error("ngm_ref_create: references >= 4 Gbp (multi-unit index) are not supported yet"); ngm_ref_destroy(r); return nullptr; }
	if (finish_ref(r) != 0) { ngm_ref_destroy(r); return nullptr; }
	return r;
}
}  // namespace

namespace ngm {
void pipeline_set_error(const char *fmt, ...) {
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_pipeline_error = buf;
}
}  // namespace ngm

extern "C" {

const char *ngm_pipeline_last_error(void) { return g_pipeline_error.c_str(); }

ngm_ref *ngm_ref_create(int device, const ngm_ref_params *p, int n_contigs, const char *const *names,
		const uint8_t *const *seqs, const uint64_t *lens) {
	ngm_ref *r = new_ref(device, p);
	if (!r) return nullptr;
	for (int i = 0; i < n_contigs; ++i) append_contig(r, names[i], seqs[i], lens[i]);
	return seal(r);
}

// NextGenMap's own cache files next to the FASTA: <ref>-enc.2.ngm (SequenceProvider.cpp:189-208, :228-262) and
// <ref>-ht-<k>-<skip>.3.ngm (PrefixTable.cpp:819-855, :857-930).  nullptr (with the reason as last error) when they are
// absent, were written with other parameters or are not single-unit indexes.
namespace {
// a cache file mapped read-only (the kernel's page cache is the only copy of its bytes on the host)
struct MappedCache {
	const uint8_t *p = nullptr;
	size_t n = 0;
	int fd = -1;
	bool open(const char *path) {
		fd = ::open(path, O_RDONLY);
		if (fd < 0) return false;
		struct stat st;
		if (fstat(fd, &st) != 0 || st.st_size <= 0) return false;
		n = (size_t) st.st_size;
		void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
		if (m == MAP_FAILED) return false;
		p = (const uint8_t *) m;
		return true;
	}
	~MappedCache() { if (p) munmap((void *) p, n); if (fd >= 0) close(fd); }
};
}  // namespace

// NextGenMap's cache files next to the FASTA: <fasta>-enc.2.ngm (SequenceProvider.cpp:189-208, :264-330) and
// <fasta>-ht-<k>-<skip>.3.ngm (PrefixTable.cpp:819-903).  Both files are mapped; everything that touches the 1.5 + 4.4 GB of a
// GRCh38-size reference (decoding, checks, the copies to the GPU) runs on all pool threads.
ngm_ref *ngm_ref_create_from_cache(int device, const ngm_ref_params *p, const char *fasta_path) {
	if (!p || !fasta_path) { ngm::pipeline_set_error("ngm_ref_create_from_cache: null argument"); return nullptr; }
	const std::string enc_fn = std::string(fasta_path) + "-enc.2.ngm";
	const std::string ht_fn = std::string(fasta_path) + "-ht-" + std::to_string(p->kmer) + "-" + std::to_string(p->kmer_skip) + ".3.ngm";
	MappedCache fe, fh;
	if (!fe.open(enc_fn.c_str()) || !fh.open(ht_fn.c_str())) { ngm::pipeline_set_error("no index cache next to %s", fasta_path); return nullptr; }
	const bool timing = getenv("NGM_HIP_HOST_TIMING") != nullptr;
	auto t0 = std::chrono::steady_clock::now();
	auto lap = [&](const char *what) {
		if (!timing) return;
		const auto t1 = std::chrono::steady_clock::now();
		fprintf(stderr, "[ngm-hip] index cache: %s %.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
		t0 = t1;
	};
	ngm_ref *r = new_ref(device, p);
	if (!r) return nullptr;
	auto fail = [&](const char *why) -> ngm_ref * { ngm::pipeline_set_error("index cache of %s: %s", fasta_path, why); ngm_ref_destroy(r); return nullptr; };
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	struct RefIdx { uint32_t SeqId, Flags; uint64_t SeqStart; uint32_t SeqLen, NameLen; char name[100]; uint32_t pad; };
	static_assert(sizeof(RefIdx) == 128, "RefIdx layout");
	size_t at = 0;
	auto take = [](const MappedCache &f, size_t &o, void *dst, size_t bytes) -> bool { if (o + bytes > f.n) return false; memcpy(dst, f.p + o, bytes); o += bytes; return true; };
	uint32_t cookie = 0, ref_count = 0;
	uint64_t bin_ref_index = 0, enc_size = 0;
	if (!take(fe, at, &cookie, 4) || !take(fe, at, &ref_count, 4) || !take(fe, at, &bin_ref_index, 8) || !take(fe, at, &enc_size, 8) ||
			cookie != 0x74656 || ref_count == 0 || bin_ref_index >= 0xFFFFFFFFull || enc_size < bin_ref_index / 2) return fail("bad header of the encoded reference");
	for (uint32_t i = 0; i < ref_count; ++i) {
		RefIdx x;
		if (!take(fe, at, &x, sizeof(x))) return fail("truncated contig table");
		NgmContig c;
		c.name.assign(x.name, std::min<uint32_t>(x.NameLen, 100));
		c.start = x.SeqStart; c.len = x.SeqLen;
		r->contigs.push_back(c);
	}
	if (at + enc_size > fe.n) return fail("truncated sequence data");
	{
		// 4 bits per base, first base in the high nibble, A0 T1 G2 C3 N4 (SequenceProvider.cpp:72-85) -> classes A0 C1 G2 T3 N5
		const uint8_t *data = fe.p + at;
		r->host_cls.resize(bin_ref_index);
		uint8_t *cls = r->host_cls.data();
		const uint64_t n_bytes = (bin_ref_index + 1) / 2;
		pool.parallel_for((int) ((n_bytes + (1u << 20) - 1) >> 20), [&](int lo, int hi) {
			static const uint8_t dec[16] = {0, 3, 2, 1, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5};
			for (uint64_t b = (uint64_t) lo << 20, e = std::min<uint64_t>(n_bytes, (uint64_t) hi << 20); b < e; ++b) {
				const uint8_t x = data[b];
				cls[2 * b] = dec[x >> 4];
				if (2 * b + 1 < bin_ref_index) cls[2 * b + 1] = dec[x & 15];
			}
		}, 1);
	}
	r->n_bases = bin_ref_index;
	lap("sequence decoded");
	uint32_t kk = 0, skip = 0, units = 0, index_size = 0, table_len = 0;
	cookie = 0;
	at = 0;
	if (!take(fh, at, &cookie, 4) || !take(fh, at, &kk, 4) || !take(fh, at, &skip, 4) || !take(fh, at, &units, 4) || !take(fh, at, &index_size, 4) ||
			!take(fh, at, &table_len, 4) || cookie != 0x74656) return fail("bad header of the k-mer table");
	const uint32_t n_kmers = 1u << (2 * p->kmer);
	if ((int) kk != p->kmer || (int) skip != p->kmer_skip || index_size != n_kmers + 1) return fail("k-mer table was built with other parameters");
	if (units != 1) return fail("multi-unit k-mer tables (references >= 4 Gbp) are not supported yet");
	const size_t ib_bytes = (size_t) index_size * 5, pos_bytes = (size_t) table_len * 4;
	if (at + ib_bytes + pos_bytes + 12 > fh.n) return fail("truncated k-mer table");
	const uint8_t *ib = fh.p + at;
	const uint8_t *pos = ib + ib_bytes;
	{
		// trailer: offset of the unit + signature (PrefixTable.cpp:838-846, checked by the reference at :892-903)
		size_t o = at + ib_bytes + pos_bytes;
		uint64_t unit_offset = 0;
		uint32_t signature = 0;
		if (!take(fh, o, &unit_offset, 8) || !take(fh, o, &signature, 4) || signature != cookie + kk + skip + units + index_size)
			return fail("k-mer table without a valid signature (truncated or written by another version)");
	}
	// a corrupt file must not turn into out-of-bounds reads on the GPU: contigs inside the encoded genome, index offsets
	// monotonic and inside the position table
	for (const NgmContig &c : r->contigs) if (c.start + c.len > bin_ref_index || c.len == 0) return fail("contig table does not match the sequence data");
	std::vector<uint32_t, ngm::default_init_allocator<uint32_t>> raw(n_kmers);
	std::vector<uint2, ngm::default_init_allocator<uint2>> idx(n_kmers);
	{
		std::atomic<bool> corrupt{false};
		auto entry = [&](uint32_t q) { uint32_t t; memcpy(&t, ib + (size_t) q * 5, 4); return t; };
		pool.parallel_for((int) ((n_kmers + (1u << 16) - 1) >> 16), [&](int lo, int hi) {
			const uint32_t a = (uint32_t) lo << 16, e = (uint32_t) std::min<uint64_t>(n_kmers, (uint64_t) hi << 16);
			uint32_t t0 = entry(a);
			if (t0 < 1u) { corrupt = true; return; }
			for (uint32_t q = a; q < e; ++q) {
				const uint32_t t1 = entry(q + 1);
				if (t1 < t0 || t1 > table_len + 1) { corrupt = true; return; }
				raw[q] = t1 - t0;
				// the usage byte doubles as "skip this k-mer" (PrefixTable.cpp:468-478, :771-775)
				idx[q] = make_uint2(t0 - 1, ib[(size_t) q * 5 + 4] ? t1 - t0 : 0u);
				t0 = t1;
			}
		}, 1);
		if (corrupt) return fail("corrupt k-mer table index");
	}
	r->n_entries = table_len;
	lap("index entries checked");
	if (upload_genome(r) != 0) { ngm_ref_destroy(r); return nullptr; }
	lap("sequence packed and copied");
	const size_t pos_alloc = ((size_t) table_len + 16) * 4;
	if (r->d_index.alloc(n_kmers) || r->d_raw_counts.alloc(n_kmers) ||
			r->d_positions.alloc((size_t) table_len + 16) || hipMemset((char *) r->d_positions.p + pos_bytes, 0, pos_alloc - pos_bytes) != hipSuccess) {
		ngm::pipeline_set_error("out of device memory loading the index cache");
		ngm_ref_destroy(r);
		return nullptr;
	}
	if (upload_staged(r->d_index.p, idx.data(), (size_t) n_kmers * 8) != 0 || upload_staged(r->d_raw_counts.p, raw.data(), (size_t) n_kmers * 4) != 0 ||
			upload_staged(r->d_positions.p, pos, pos_bytes) != 0) { ngm_ref_destroy(r); return nullptr; }
	lap("k-mer table copied");
	index_stats(r, raw.data(), n_kmers);
	r->from_cache = true;
	return r;
}

static ngm_ref *create_from_fasta(int device, const ngm_ref_params *p, const char *path, const char *vcf_path) {
	// like the reference, an index cache next to the FASTA is used instead of rebuilding (NGM_HIP_NO_CACHE=1: always rebuild); the
	// VCF is then not read at all (PrefixTable.cpp:223-228 only reads it when the table is built)
	if (!getenv("NGM_HIP_NO_CACHE")) {
		if (ngm_ref *cached = ngm_ref_create_from_cache(device, p, path)) return cached;
	}
	if (vcf_path) {  // an unreadable VCF is an error before any GPU work (the reference logs it and goes on without variants)
		gzFile v = gzopen(vcf_path, "rb");
		if (!v) { ngm::pipeline_set_error("Failed to open VCF file %s", vcf_path); return nullptr; }
		gzclose(v);
	}
	gzFile f = gzopen(path, "rb");
	if (!f) { ngm::pipeline_set_error("cannot open reference %s", path); return nullptr; }
	ngm_ref *r = new_ref(device, p);
	if (!r) { gzclose(f); return nullptr; }
	std::string name, seq, line;
	bool have = false;
	std::vector<char> buf(1 << 20);
	std::string carry;
	auto flush = [&]() { if (have) append_contig(r, name, (const uint8_t *) seq.data(), seq.size()); seq.clear(); };
	auto handle_line = [&](const char *s, size_t n) {
		while (n && (s[n - 1] == '\r' || s[n - 1] == '\n')) --n;
		if (n && s[0] == '>') {
			flush();
			size_t e = 1;
			while (e < n && s[e] != ' ' && s[e] != '\t') ++e;  // kseq: name = up to the first whitespace
			name.assign(s + 1, e - 1);
			have = true;
		} else if (have) {
			for (size_t i = 0; i < n; ++i) if (s[i] != ' ' && s[i] != '\t') seq.push_back(s[i]);
		}
	};
	int got;
	while ((got = gzread(f, buf.data(), (unsigned) buf.size())) > 0) {
		size_t b = 0;
		for (size_t i = 0; i < (size_t) got; ++i) {
			if (buf[i] == '\n') {
				if (!carry.empty()) { carry.append(buf.data() + b, i - b); handle_line(carry.data(), carry.size()); carry.clear(); }
				else handle_line(buf.data() + b, i - b);
				b = i + 1;
			}
		}
		carry.append(buf.data() + b, (size_t) got - b);
	}
	if (!carry.empty()) handle_line(carry.data(), carry.size());
	flush();
	gzclose(f);
	NgmVcf vcf;
	if (vcf_path) {
		if (ngm_vcf_read(vcf_path, r->contigs, vcf) != 0) { ngm_ref_destroy(r); return nullptr; }
		r->vcf = &vcf;
	}
	ngm_ref *out = seal(r);
	if (out) out->vcf = nullptr;  // (the variants live in the index now)
	return out;
}

ngm_ref *ngm_ref_create_from_fasta(int device, const ngm_ref_params *p, const char *path) { return create_from_fasta(device, p, path, nullptr); }

ngm_ref *ngm_ref_create_from_fasta_vcf(int device, const ngm_ref_params *p, const char *fasta_path, const char *vcf_path) {
	if (!vcf_path) { ngm::pipeline_set_error("ngm_ref_create_from_fasta_vcf: no VCF file given"); return nullptr; }
	return create_from_fasta(device, p, fasta_path, vcf_path);
}

int ngm_ref_vcf_summary(const ngm_ref *r, uint64_t out[6]) {
	if (!r || !out) return -22;
	for (int i = 0; i < 6; ++i) out[i] = r->vcf_summary[i];
	return r->vcf_applied ? 1 : 0;
}

int ngm_ref_vcf_skip_counts(const ngm_ref *r, uint64_t out[2]) {
	if (!r || !out) return -22;
	out[0] = r->vcf_skip_count; out[1] = r->vcf_skip_build;
	return r->vcf_applied ? 1 : 0;
}

void ngm_ref_destroy(ngm_ref *r) {
	if (!r) return;
	(void) hipSetDevice(r->device);
	delete r;
}

}  // extern "C"

int ngm_ref_ensure_buckets(const ngm_ref *r, int kind) {
	std::lock_guard<std::mutex> lk(g_bucket_mu);
	int prev = -1;
	(void) hipGetDevice(&prev);
	(void) hipSetDevice(r->device);
	const int rc = build_buckets_kind(const_cast<ngm_ref *>(r), kind);
	if (prev >= 0 && prev != r->device) (void) hipSetDevice(prev);
	return rc;
}

extern "C" {

int ngm_ref_prepare_search(ngm_ref *r, int bs_mapping) {
	if (!r) return -22;
	if (bs_mapping) return 0;
	const bool canon = (r->prm.kmer & 1) != 0;   // (mapper.cpp: reads of more than 256 k-mers fall back to one bucket per k-mer)
	return ngm_ref_ensure_buckets(r, canon ? 1 : 0);
}

int ngm_ref_host_classes(const ngm_ref *r, uint64_t pos, int n, uint8_t *out) {
	if (!r || !out || n < 0) return -22;
	int k = 0;
	for (; k < n && pos + (uint64_t) k < r->host_cls.size(); ++k) out[k] = r->host_cls[pos + (uint64_t) k];
	return k;
}

int ngm_ref_contig_count(const ngm_ref *r) { return (int) r->contigs.size(); }
const char *ngm_ref_contig_name(const ngm_ref *r, int i) { return r->contigs[i].name.c_str(); }
uint64_t ngm_ref_contig_start(const ngm_ref *r, int i) { return r->contigs[i].start; }
uint64_t ngm_ref_contig_len(const ngm_ref *r, int i) { return r->contigs[i].len; }
uint64_t ngm_ref_concat_len(const ngm_ref *r) { return r->n_bases - 1; }  // SequenceProvider.cpp:454-456
int ngm_ref_auto_max_kfreq(const ngm_ref *r) { return r->auto_max_kfreq; }
int ngm_ref_loaded_from_cache(const ngm_ref *r) { return r->from_cache ? 1 : 0; }
uint64_t ngm_ref_index_entries(const ngm_ref *r) { return r->n_entries; }

int ngm_ref_index_copy(const ngm_ref *r, uint32_t *counts, uint32_t *raw_counts, uint32_t *positions) {
	(void) hipSetDevice(r->device);
	const uint32_t n_kmers = 1u << (2 * r->prm.kmer);
	if (counts) {
		std::vector<uint2> idx(n_kmers);
		REF_HIP_TRY(hipMemcpy(idx.data(), r->d_index.p, (size_t) n_kmers * sizeof(uint2), hipMemcpyDeviceToHost));
		for (uint32_t i = 0; i < n_kmers; ++i) counts[i] = idx[i].y;
	}
	if (raw_counts) REF_HIP_TRY(hipMemcpy(raw_counts, r->d_raw_counts.p, (size_t) n_kmers * 4, hipMemcpyDeviceToHost));
	if (positions && r->n_entries) REF_HIP_TRY(hipMemcpy(positions, r->d_positions.p, r->n_entries * 4, hipMemcpyDeviceToHost));
	return 0;
}

// A cache file appears under its name complete or not at all: it is written to <name>.tmp.<pid>, every write is checked, and then
// renamed (another process -- a sibling shard, another run -- may be mapping the old file while this one is written)
namespace {
struct CacheFile {
	std::string fn, tmp;
	FILE *fp = nullptr;
	bool ok = true;
	explicit CacheFile(const std::string &name) : fn(name), tmp(name + ".tmp." + std::to_string((long) getpid())) { fp = fopen(tmp.c_str(), "wb"); ok = fp != nullptr; }
	void put(const void *p, size_t size, size_t n) { if (ok && n && fwrite(p, size, n, fp) != n) ok = false; }
	bool commit() {
		if (fp && fclose(fp) != 0) ok = false;
		fp = nullptr;
		if (ok && rename(tmp.c_str(), fn.c_str()) != 0) ok = false;
		if (!ok) (void) unlink(tmp.c_str());
		return ok;
	}
	~CacheFile() { if (fp) { fclose(fp); (void) unlink(tmp.c_str()); } }
};
}  // namespace

int ngm_ref_write_ngm_cache(const ngm_ref *r, const char *fasta_path) {
	(void) hipSetDevice(r->device);
	const int k = r->prm.kmer;
	const uint32_t n_kmers = 1u << (2 * k);
	// ---- <ref>-enc.2.ngm -------------------------------------------------------------------------------
	{
		const std::string fn = std::string(fasta_path) + "-enc.2.ngm";
		CacheFile cf(fn);
		if (!cf.ok) { ngm::pipeline_set_error("cannot write %s", fn.c_str()); return -13; }
		const uint32_t cookie = 0x74656, ref_count = (uint32_t) r->contigs.size();
		uint64_t size = 1000;  // getSize(): SequenceProvider.cpp:210-226
		for (const NgmContig &c : r->contigs) size += ((c.len | 1) + 1) + 1000;
		const uint64_t bin_ref_index = r->n_bases, enc_size = ((size / 2) | 1) + 1;
		cf.put(&cookie, 4, 1); cf.put(&ref_count, 4, 1); cf.put(&bin_ref_index, 8, 1); cf.put(&enc_size, 8, 1);
		struct RefIdx { uint32_t SeqId, Flags; uint64_t SeqStart; uint32_t SeqLen, NameLen; char name[100]; uint32_t pad; };
		static_assert(sizeof(RefIdx) == 128, "RefIdx layout");
		for (size_t i = 0; i < r->contigs.size(); ++i) {
			RefIdx x{};
			x.SeqId = (uint32_t) i; x.SeqStart = r->contigs[i].start; x.SeqLen = (uint32_t) r->contigs[i].len;
			x.NameLen = (uint32_t) std::min<size_t>(100, r->contigs[i].name.size());
			memcpy(x.name, r->contigs[i].name.data(), x.NameLen);
			cf.put(&x, sizeof(x), 1);
		}
		// 4 bits per base, first base in the high nibble, A0 T1 G2 C3 N4 (SequenceProvider.cpp:72-85, :310-313)
		static const uint8_t enc[8] = {0, 3, 2, 1, 4, 4, 4, 4};
		std::vector<uint8_t> data(enc_size, 0);
		for (uint64_t i = 0; i + 1 < r->n_bases; i += 2) data[i >> 1] = (uint8_t) ((enc[r->host_cls[i] & 7] << 4) | enc[r->host_cls[i + 1] & 7]);
		cf.put(data.data(), 1, enc_size);
		if (!cf.commit()) { ngm::pipeline_set_error("write error on %s", fn.c_str()); return -5; }
	}
	// ---- <ref>-ht-<k>-<skip>.3.ngm ---------------------------------------------------------------------
	{
		const std::string fn = std::string(fasta_path) + "-ht-" + std::to_string(k) + "-" + std::to_string(r->prm.kmer_skip) + ".3.ngm";
		CacheFile cf(fn);
		if (!cf.ok) { ngm::pipeline_set_error("cannot write %s", fn.c_str()); return -13; }
		const uint32_t cookie = 0x74656, kk = (uint32_t) k, skip = (uint32_t) r->prm.kmer_skip, units = 1, index_size = n_kmers + 1;
		cf.put(&cookie, 4, 1); cf.put(&kk, 4, 1); cf.put(&skip, 4, 1); cf.put(&units, 4, 1); cf.put(&index_size, 4, 1);
		std::vector<uint32_t> raw(n_kmers);
		std::vector<uint2> idx(n_kmers);
		REF_HIP_TRY(hipMemcpy(raw.data(), r->d_raw_counts.p, (size_t) n_kmers * 4, hipMemcpyDeviceToHost));
		REF_HIP_TRY(hipMemcpy(idx.data(), r->d_index.p, (size_t) n_kmers * 8, hipMemcpyDeviceToHost));
		std::vector<uint32_t> pos(r->n_entries + 1, 0);
		if (r->n_entries) REF_HIP_TRY(hipMemcpy(pos.data(), r->d_positions.p, r->n_entries * 4, hipMemcpyDeviceToHost));
		const uint32_t table_len = (uint32_t) r->n_entries;
		cf.put(&table_len, 4, 1);
		// Index { uint m_TabIndex; char m_RevCompIndex; } packed to 5 bytes (PrefixTable.h:18-61)
		std::vector<uint8_t> ib((size_t) index_size * 5, 0);
		uint32_t next = 0;
		for (uint32_t p = 0; p < n_kmers; ++p) {
			const uint32_t tab = next + 1;
			memcpy(&ib[(size_t) p * 5], &tab, 4);
			if (raw[p] > 0) {
				const uint32_t total = raw[p] + raw[ngm::kmer_revcomp(p, k)];
				const int dummy = 10000;
				ib[(size_t) p * 5 + 4] = (uint8_t) (char) ((dummy - (int) std::min<uint32_t>(total, dummy)) * 100.0f / dummy);
				if (idx[p].y == 0) for (uint32_t j = 0; j < raw[p]; ++j) pos[next + j] = 0;  // unused k-mers keep empty slots
			}
			next += raw[p];
		}
		const uint32_t tab = next + 1;
		memcpy(&ib[(size_t) n_kmers * 5], &tab, 4);
		cf.put(ib.data(), 1, ib.size());
		cf.put(pos.data(), 4, table_len);
		const uint64_t offset = 0;
		cf.put(&offset, 8, 1);
		const uint32_t signature = cookie + kk + skip + units + index_size;
		cf.put(&signature, 4, 1);
		if (!cf.commit()) { ngm::pipeline_set_error("write error on %s", fn.c_str()); return -5; }
	}
	return 0;
}

// _SequenceProvider::convert (SequenceProvider.cpp:111-141)
int ngm_ref_convert(const ngm_ref *r, uint64_t pos, int *contig, uint64_t *contig_pos) {
	auto upper = std::upper_bound(r->start_pos.begin(), r->start_pos.end(), pos);
	if (upper == r->start_pos.end() || upper == r->start_pos.begin()) return 0;
	if ((*upper - pos) < 1000) return 0;  // inside the spacer in front of the next contig
	*contig = (int) ((upper - 1) - r->start_pos.begin());
	*contig_pos = pos - *(upper - 1);
	return 1;
}

}  // extern "C"
