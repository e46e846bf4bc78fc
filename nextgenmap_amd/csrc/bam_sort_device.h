// bam_sort_device.h -- the kernels of `ngm-hip --sort` (csrc/bam_sort.cpp): record offsets from ranges, keys from records, the byte-granular
// gather of the sorted records into the stream the BGZF compressor reads, and the arrays of the BAI file.  DESIGN.md section 4.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bam_sort.h"

namespace ngm {
namespace bamsort {

// what the key kernel refuses (ngm_bam_sort_finish names the first such record)
enum { kBadRef = 1, kBadPos = 2, kBadEnd = 3 };

// ---- record offsets ----------------------------------------------------------------------------------------------------------------------
// A thread walks the records of its range [off[i], off[i + 1]) -- 256 records noted by the host's walk, or a unit of the device formatter
// (0, 1 or 2 records).  Every record is checked before its fields are read (check_record); a range that does not end exactly at its end
// reports itself in *bad (the smallest such range) and is cut there.  WRITE = false: count[i] = records; WRITE = true: rec_off[base[i] + k] (below cap).
template <bool WRITE>
__global__ __launch_bounds__(256) void walk_ranges_kernel(const uint8_t *seg, const uint32_t *off, uint32_t n_ranges, uint32_t *count, const uint32_t *base, uint32_t *rec_off,
		uint32_t cap /* entries of rec_off */, uint32_t *bad) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n_ranges) return;
	uint32_t at = off[i];
	const uint32_t end = off[i + 1];
	uint32_t k = 0;
	const uint32_t b = WRITE ? base[i] : 0u;
	while (at < end) {
		uint32_t size = 0;
		if (check_record(seg + at, (uint64_t) (end - at), &size) != kOk) { atomicMin(bad, i); break; }
		if (WRITE && b + k < cap) rec_off[b + k] = at;
		at += size;
		++k;
	}
	if (!WRITE) count[i] = k;
}

// ---- keys --------------------------------------------------------------------------------------------------------------------------------
// One thread per record of a segment (records g0 .. g0 + n of the run order): key, its place, address, length, end on the reference and
// bin << 1 | flag 4.  Reads the fixed part and the CIGAR only: offsets the walk has validated.  *bad: (record << 8 | reason) of the first
// record finish must refuse; *n_no_coor counts refID < 0.
__global__ __launch_bounds__(256) void keys_kernel(const uint8_t *seg, const uint32_t *rec_off, uint32_t n, uint64_t g0, int n_ref, uint64_t *key, uint32_t *idx,
		uint64_t *ptr, uint32_t *len, uint32_t *end_out, uint32_t *bin_flag, unsigned long long *bad, unsigned long long *n_no_coor) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool live = i < n;
	bool no_coor = false;
	if (live) {
		const uint8_t *p = seg + rec_off[i];
		const int32_t ref_id = (int32_t) ld32(p + 4), pos = (int32_t) ld32(p + 8);
		const uint32_t flag = ld32(p + 16) >> 16;
		const uint64_t g = g0 + i;
		int why = 0;
		int64_t end = 0;
		uint32_t bin = 0;
		if (ref_id < -1 || ref_id >= n_ref) why = kBadRef;
		else if (ref_id >= 0) {
			if (pos < 0) why = kBadPos;
			else {
				end = record_end(p);
				if (end > kMaxEnd) why = kBadEnd;
				else bin = reg2bin(pos, end);
			}
		} else no_coor = true;
		if (why) atomicMin(bad, (unsigned long long) ((g << 8) | (uint64_t) why));
		key[g] = sort_key(ref_id, pos, flag);
		idx[g] = (uint32_t) g;
		ptr[g] = (uint64_t) (uintptr_t) p;
		len[g] = ld32(p) + 4u;
		end_out[g] = (uint32_t) end;
		bin_flag[g] = (bin << 1) | ((flag >> 2) & 1u);
	}
	const unsigned long long m = __ballot(no_coor);
	if (m && (threadIdx.x & 63u) == (uint32_t) (__ffsll((long long) m) - 1)) atomicAdd(n_no_coor, (unsigned long long) __popcll(m));
}

// the per-record arrays in sorted order
__global__ __launch_bounds__(256) void permute_kernel(const uint32_t *idx, uint64_t n, const uint64_t *ptr, const uint32_t *len, const uint32_t *end_in, const uint32_t *bin_flag,
		uint64_t *s_ptr, uint64_t *s_len, uint32_t *s_end, uint32_t *s_bin_flag) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= n) return;
	const uint32_t i = idx[r];
	s_ptr[r] = ptr[i]; s_len[r] = len[i]; s_end[r] = end_in[i]; s_bin_flag[r] = bin_flag[i];
}

// ---- the gather --------------------------------------------------------------------------------------------------------------------------
// Bytes [s0, s0 + n_bytes) of the sorted stream into dst (16-byte aligned; s0 is a multiple of kMember, hence of 16).  Driven from the
// destination: a lane owns one 16-byte row, a wave a tile of 1 024 consecutive bytes (and several consecutive tiles in turn).  The wave finds
// the record that holds its tile's first byte -- for its first tile by a bisection over the stream offsets u[0 .. n_rec] (the same addresses
// for all lanes: one fetch each), for the later ones in LDS, see below -- puts the next 65 offsets and 65
// addresses into LDS -- records are at least 36 bytes, so those cover the wave's bytes -- and every lane finds its row's record there in six
// steps.  A row inside one record is four aligned dwords (a fifth when the source is not dword aligned) funnel-shifted into one 16-byte
// store; a row across a record boundary, or the stream's last row, goes byte by byte.  The aligned dwords may start up to 3 bytes before a
// record and end up to 3 bytes after it: inside the segment, which starts 256-byte aligned and ends with 16 bytes of padding.
constexpr int kGatherWaves = 4, kGatherWaveBytes = 1024, kGatherBlockBytes = kGatherWaves * kGatherWaveBytes;
__global__ __launch_bounds__(256) void gather_kernel(const uint64_t *u, const uint64_t *s_ptr, uint64_t n_rec, uint64_t s0, uint64_t n_bytes, uint8_t *dst) {
	__shared__ uint64_t su[kGatherWaves][65], sp[kGatherWaves][65];
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	// a wave owns `rounds` consecutive tiles of 1 024 bytes: it bisects u[] for its first tile only (21 dependent loads for 2 M records --
	// the latency that bounded this kernel when every tile paid it); the next tile starts 1 024 bytes on, inside what
	// the 65 offsets in LDS cover (the record at [0] holds the old first byte, the 63 after it are at least 36 bytes each), so its record
	// comes from the same six-step search there
	const uint64_t n_tiles = (n_bytes + kGatherWaveBytes - 1) / kGatherWaveBytes;
	const uint64_t rounds = (n_tiles + (uint64_t) gridDim.x * kGatherWaves - 1) / ((uint64_t) gridDim.x * kGatherWaves);
	const uint64_t tile0 = ((uint64_t) blockIdx.x * kGatherWaves + w) * rounds;
	uint64_t lo = 0;
	for (uint64_t r = 0; r < rounds; ++r) {   // (the same trip count for every block: the barriers below are uniform)
		const uint64_t wave_base = (tile0 + r) * kGatherWaveBytes;
		const bool wave_live = wave_base < n_bytes;
		if (wave_live) {
			const uint64_t d0 = s0 + wave_base;
			if (r == 0) {
				uint64_t hi = n_rec;   // u[lo] <= d0 < u[hi]: u[0] = 0, u[n_rec] = the stream's length
				while (hi - lo > 1) {
					const uint64_t mid = lo + (hi - lo) / 2;
					if (u[mid] <= d0) lo = mid; else hi = mid;
				}
			} else {
				uint32_t j = 0;
#pragma unroll
				for (uint32_t step = 32; step; step >>= 1) if (su[w][j + step] <= d0) j += step;
				lo += j;
			}
			const uint64_t a = lo + lane;
			const uint64_t ua = a <= n_rec ? u[a] : ~0ull, pa = a < n_rec ? s_ptr[a] : 0ull;
			const uint64_t u64 = lo + 64 <= n_rec ? u[lo + 64] : ~0ull, p64 = lo + 64 < n_rec ? s_ptr[lo + 64] : 0ull;
			su[w][lane] = ua;
			sp[w][lane] = pa;
			if (lane == 0) { su[w][64] = u64; sp[w][64] = p64; }
		}
		__syncthreads();
		const uint64_t row = wave_base + (uint64_t) lane * 16u;
		if (wave_live && row < n_bytes) {
			const uint64_t d = s0 + row;
			uint32_t j = 0;
#pragma unroll
			for (uint32_t step = 32; step; step >>= 1) if (su[w][j + step] <= d) j += step;
			const uint64_t left = n_bytes - row;
			uint8_t *out = dst + row;
			if (su[w][j + 1] - d >= 16 && left >= 16) {
				const uint64_t src = sp[w][j] + (d - su[w][j]);
				const uint32_t sh = (uint32_t) (src & 3u);
				const uint32_t *q = (const uint32_t *) (uintptr_t) (src - sh);
				const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = sh ? q[4] : 0u;
				uint4 v;
				v.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
				v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
				v.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
				v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
				*(uint4 *) out = v;
			} else {
				const uint32_t nb = left < 16 ? (uint32_t) left : 16u;
				for (uint32_t b = 0; b < nb; ++b) {
					while (j < 64 && su[w][j + 1] <= d + b) ++j;
					out[b] = *(const uint8_t *) (uintptr_t) (sp[w][j] + (d + b - su[w][j]));
				}
			}
		}
		__syncthreads();
	}
}

// ---- the index ---------------------------------------------------------------------------------------------------------------------------
struct IndexArgs {
	uint64_t n_coor;            // the sorted records with a reference: the first n_coor
	const uint64_t *key;        // sorted keys
	const uint64_t *u;          // stream offsets [n + 1]
	const uint32_t *s_end, *s_bin_flag;
	const uint64_t *C;          // compressed bytes in front of member k [members + 1]
	uint64_t first;             // file offset of the first member
	uint64_t *vbeg, *vend;      // per record
	uint32_t *head;             // [n_coor + 1]: 1 where a chunk starts (a new reference or bin); the last entry 0
	unsigned long long *ref_vbeg, *ref_vend, *ref_first, *ref_last, *ref_unmapped, *ref_maxend;   // per reference
};

// per record: virtual offsets, chunk heads, what its reference keeps of it.  The largest end of a reference is at its last record or at a
// record whose successor ends earlier: only those take the atomic.
__global__ __launch_bounds__(256) void index_records_kernel(IndexArgs A) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= A.n_coor) return;
	const uint32_t ref = (uint32_t) (A.key[r] >> 32), bf = A.s_bin_flag[r];
	const uint64_t vb = virtual_offset(A.u[r], A.first, A.C), ve = virtual_offset(A.u[r + 1], A.first, A.C);
	A.vbeg[r] = vb; A.vend[r] = ve;
	const bool ref_head = r == 0 || (uint32_t) (A.key[r - 1] >> 32) != ref;
	const bool ref_tail = r + 1 == A.n_coor || (uint32_t) (A.key[r + 1] >> 32) != ref;
	A.head[r] = (ref_head || (A.s_bin_flag[r - 1] >> 1) != (bf >> 1)) ? 1u : 0u;
	if (r + 1 == A.n_coor) A.head[r + 1] = 0u;
	if (ref_head) { A.ref_vbeg[ref] = vb; A.ref_first[ref] = r; }
	if (ref_tail) { A.ref_vend[ref] = ve; A.ref_last[ref] = r + 1; }
	if (bf & 1u) atomicAdd(A.ref_unmapped + ref, 1ull);
	if (ref_tail || A.s_end[r] > A.s_end[r + 1]) atomicMax(A.ref_maxend + ref, (unsigned long long) A.s_end[r]);
}

// chunk c = the run of records that starts at the c-th head: (reference << 32 | bin, vbeg of its first record, vend of its last)
__global__ __launch_bounds__(256) void chunks_kernel(IndexArgs A, const uint32_t *before /* heads in front of r */, uint64_t *ckey, uint32_t *cval, uint64_t *cbeg, uint64_t *cend) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= A.n_coor) return;
	const uint32_t h = A.head[r], c = before[r] + h - 1u;
	if (h) { ckey[c] = (A.key[r] & 0xFFFFFFFF00000000ull) | (A.s_bin_flag[r] >> 1); cval[c] = c; cbeg[c] = A.vbeg[r]; }
	if (r + 1 == A.n_coor || A.head[r + 1]) cend[c] = A.vend[r];
}

__global__ __launch_bounds__(256) void chunks_permute_kernel(const uint32_t *order, uint64_t n, const uint64_t *cbeg, const uint64_t *cend, uint64_t *s_beg, uint64_t *s_end) {
	const uint64_t c = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (c >= n) return;
	s_beg[c] = cbeg[order[c]]; s_end[c] = cend[order[c]];
}

// windows of 16 384 bases per reference: ((largest end - 1) >> 14) + 1, none without records; and the records per reference by flag 4
__global__ __launch_bounds__(256) void ref_windows_kernel(int n_ref, const unsigned long long *ref_maxend, const unsigned long long *ref_first, const unsigned long long *ref_last,
		const unsigned long long *ref_unmapped, uint64_t *n_intv, uint64_t *ref_mapped) {
	const int r = (int) (blockIdx.x * 256u + threadIdx.x);
	if (r > n_ref) return;
	if (r == n_ref) { n_intv[r] = 0; return; }
	n_intv[r] = ref_maxend[r] ? ((ref_maxend[r] - 1) >> 14) + 1 : 0;
	ref_mapped[r] = ref_last[r] - ref_first[r] - ref_unmapped[r];
}

// ioffset: the smallest vbeg of the records that overlap a window.  The records arrive sorted, so the first record to reach a window wins;
// a record leaves out the windows its predecessor (same reference) covers as well -- that one starts no later.  The array is kept back to
// front (rev[n_win - 1 - i]) so that a forward min-scan fills an empty window with the value of the next one that has a record.
__global__ __launch_bounds__(256) void windows_kernel(IndexArgs A, const uint64_t *win_base, uint64_t n_win, unsigned long long *rev) {
	const uint64_t r = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (r >= A.n_coor) return;
	const uint32_t ref = (uint32_t) (A.key[r] >> 32);
	const uint32_t beg = (uint32_t) ((A.key[r] >> 1) & 0x7fffffffu) - 1u, end = A.s_end[r];
	uint32_t w0 = beg >> 14;
	const uint32_t w1 = (end - 1u) >> 14;
	if (r > 0 && (uint32_t) (A.key[r - 1] >> 32) == ref) {
		const uint32_t pw1 = (A.s_end[r - 1] - 1u) >> 14;   // (the predecessor starts at or before beg)
		if (pw1 >= w0) w0 = pw1 + 1u;
	}
	const uint64_t base = win_base[ref];
	for (uint32_t w = w0; w <= w1 && w1 != 0xFFFFFFFFu; ++w) atomicMin(rev + (n_win - 1 - (base + w)), (unsigned long long) A.vbeg[r]);
}

__global__ __launch_bounds__(256) void reverse_kernel(const uint64_t *in, uint64_t n, uint64_t *out) {
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (i < n) out[i] = in[n - 1 - i];
}

}  // namespace bamsort
}  // namespace ngm
