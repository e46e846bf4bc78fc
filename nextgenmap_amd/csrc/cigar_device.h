// cigar_device.h -- CIGAR / MD / NM / Identity of a batch of alignments on the GPU.
// Device twin of cigar_md.h: SWOclCigar::computeCigarMD (lib/mason/opencl/SWOclCigar.cpp:430-615) for the default
// personality, EndToEndAffine::convertToCIGAR (src/seqan/EndToEndAffine.cpp:52-155) for `--affine`.  The host versions
// stay as the reference for tests and as the fall-back for strings that do not fit the scratch rows; what moves here is the
// part that hurt on the host: the MD string needs the reference window, which is already in HBM (the packed pairs of the
// align stage) but costs three cache-missing reads into a 3 GB array per read on the host.
// One lane per alignment; the packed pairs are 64-way interleaved, so a wave's lanes read consecutive dwords.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_device.h"
#include "affine_device.h"

namespace ngm {

struct CigarDevOut {   // per alignment
	uint32_t cig_off, md_off;     // into the compact byte stream
	uint16_t cig_len, md_len;     // bytes, without the terminating NUL
	int32_t position_offset, qstart, qend, nm;
	float identity, score_token;
	int32_t flags;                // bit 0: strings valid (else: host fall-back), bit 1: alignment valid (linear: rec[0])
};

__device__ __forceinline__ uint32_t packed_class(const uint32_t *base, int m_base, int j) {  // symbol j of a 64-way interleaved row
	const uint32_t w = base[(size_t) (m_base + (j >> 3)) * kSlots];
	const int b = j & 7;
	return (b < 4) ? (w >> (8 * b)) & 15u : (w >> (8 * (b - 4) + 4)) & 15u;
}
__device__ __forceinline__ char class_to_char(uint32_t c) {
	switch (c) { case 0: return 'A'; case 1: return 'C'; case 2: return 'G'; case 3: return 'T'; case 4: return 'x'; case 5: return 'N'; default: return 0; }
}
__device__ __forceinline__ int dev_put_num(char *dst, int v) {
	char b[12];
	int n = 0, i = 0;
	unsigned u = v < 0 ? 0u - (unsigned) v : (unsigned) v;
	if (v < 0) dst[i++] = '-';
	do { b[n++] = (char) ('0' + u % 10u); u /= 10u; } while (u);
	while (n) dst[i++] = b[--n];
	return i;
}

// cig / md: scratch rows of `stride` bytes per alignment.  read_len: per READ (affine: QEnd); a_read: read of alignment j.
// The strings are built in LDS rows (kCigarRow bytes for the CIGAR, as many for MD -- byte stores to 608-byte-strided global rows
// cost one cache line per lane and store) and leave the workgroup as one contiguous piece of the compact byte stream: block
// prefix sum of the lengths, ONE atomic on the stream cursor per workgroup.
constexpr int kCigarRow = 96;

template <bool AFFINE>
__global__ __launch_bounds__(256) void cigar_strings_kernel(int n, const int32_t *__restrict__ records, const uint16_t *__restrict__ runs_c,
		const uint32_t *__restrict__ packed, int RW, int FW, const uint16_t *__restrict__ read_len, const uint32_t *__restrict__ a_read, int variant_cpu,
		int hard_clip, int silent_clip, CigarDevOut *__restrict__ out, char *__restrict__ bytes, unsigned long long capacity, unsigned long long *__restrict__ cursor, int alt = 0) {
	__shared__ char s_rows[256 * 2 * kCigarRow];
	__shared__ uint32_t s_wave[4];
	__shared__ unsigned long long s_base;
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = j < n;
	constexpr int stride = kCigarRow;
	CigarDevOut o{};
	char *cg = s_rows + (size_t) threadIdx.x * 2 * kCigarRow, *mdp = cg + kCigarRow;
	const int lim = stride - 16;  // room for one more element; longer strings go to the host fall-back
	bool fits = true;
	int co = 0, mo = 0;
	if (live) {
	const int32_t *rec = records + (size_t) j * 8;
	const uint16_t *runs = runs_c + (uint32_t) rec[6];
	if (AFFINE) {
		int h = rec[1], v = rec[2], total = 0, pattern_chars = 0;
		o.position_offset = h; o.qstart = v;
		if (v > 0) { co += dev_put_num(cg + co, v); cg[co++] = 'S'; }
		for (int k = rec[4] - 1; k >= 0; --k) {
			const int op = runs[k] & 3, run = runs[k] >> 2;
			if (co > lim) { fits = false; break; }
			co += dev_put_num(cg + co, run);
			if (op == 1) { total += run; h += run; v += run; pattern_chars += run; cg[co++] = 'M'; }
			else if (op == 2) { total += 1; v += run; pattern_chars += run; cg[co++] = 'I'; }
			else { total += 1; h += run; cg[co++] = 'D'; }
		}
		const int len_v = (int) read_len[a_read[j]];
		o.qend = len_v - (pattern_chars + o.qstart);
		if (co > lim) fits = false;
		if (fits && o.qend > 0) { co += dev_put_num(cg + co, o.qend); cg[co++] = 'S'; }
		o.identity = (float) rec[3] * 1.0f / (float) total;
		o.nm = rec[7];
		o.score_token = 0.f;
		mdp[0] = '!'; mdp[1] = '!'; mdp[2] = '!'; mo = 3;  // EndToEndAffine never touches pBuffer2 (AlignmentBuffer.cpp:109)
		o.flags = (fits ? 1 : 0) | 2;
	} else {
		if (!rec[0]) {  // no alignment could be built: Score = -1 (SWOclCigar.cpp:322-327)
			o.score_token = -1.0f; o.flags = 1;
		} else {
			const uint32_t *pb = packed + (size_t) (j >> 6) * (RW + FW) * kSlots + (j & 63);
			const int lead = rec[2], trail = rec[3], nruns = rec[4], ref0 = rec[1];
			if (lead > 0) {
				if (hard_clip == 1) { co += dev_put_num(cg + co, lead); cg[co++] = 'H'; }
				else if (silent_clip != 1) { co += dev_put_num(cg + co, lead); cg[co++] = 'S'; }
				o.qstart = lead;
			}
			// symbol classes of read position j / window position j: eight per dword, the dword kept while it lasts
			uint32_t rw_at = 0xFFFFFFFFu, rw = 0, fw_at = 0xFFFFFFFFu, fw = 0;
			auto nib = [](uint32_t w, int b) -> uint32_t { return (b < 4) ? (w >> (8 * b)) & 15u : (w >> (8 * (b - 4) + 4)) & 15u; };
			// (bit 3 of a read class = the pair's score table, SwConst::alt)
			auto rclass = [&](int j) -> uint32_t { const uint32_t wi = (uint32_t) j >> 3; if (wi != rw_at) { rw = pb[(size_t) wi * kSlots]; rw_at = wi; } return nib(rw, j & 7) & 7u; };
			const uint32_t dir = alt ? ((pb[0] >> 3) & 1u) : 0u;
			// bs_mapping / slam_seq: the conversion that counts as a match (SWOclCigar.cpp:300-317), as symbol classes A0 C1 G2 T3
			const uint32_t bs_from = alt == 1 ? (dir ? 0u : 3u) : (dir ? 2u : 1u), bs_to = alt == 1 ? (dir ? 2u : 1u) : (dir ? 0u : 3u);
			auto fclass = [&](int j) -> uint32_t { const uint32_t wi = (uint32_t) j >> 3; if (wi != fw_at) { fw = pb[(size_t) (RW + wi) * kSlots]; fw_at = wi; } return nib(fw, j & 7); };
			int match = 0, mismatch = 0, total = 0, m_len = 0, md_eq = 0, ref_i = 0, read_i = o.qstart;
			bool in_x_run = false, odd_symbol = false;
			for (int k = nruns - 1; k >= 0 && fits; --k) {
				const int op = runs[k] & 3, len = runs[k] >> 2;
				total += len;
				if (co > lim || mo > lim) { fits = false; break; }
				if (op == 1 || op == 0) {
					for (int t = 0; t < len; ++t) {
						const uint32_t rc = rclass(read_i), fc = fclass(ref0 + ref_i);
						if (rc == 4u) odd_symbol = true;  // a read symbol outside ACGTN: characters and classes may disagree -> host
						const bool eq = (op == 1) && ((variant_cpu && !alt) ? (rc <= 3u && rc == fc) : (rc == fc));
						if (eq) { match += 1; md_eq += 1; in_x_run = false; }
						else {
							if (alt && rc == bs_from && fc == bs_to) match += 1; else mismatch += 1;   // SWOclCigar.cpp:507-514
							if (mo > lim) { fits = false; break; }
							if (!in_x_run) { mo += dev_put_num(mdp + mo, md_eq); md_eq = 0; in_x_run = true; }
							mdp[mo++] = class_to_char(fc);
						}
						m_len += 1; ref_i += 1; read_i += 1;
					}
				} else if (op == 3) {
					in_x_run = false;
					if (m_len > 0) { co += dev_put_num(cg + co, m_len); cg[co++] = 'M'; m_len = 0; }
					co += dev_put_num(cg + co, len); cg[co++] = 'D';
					mo += dev_put_num(mdp + mo, md_eq); md_eq = 0;
					mdp[mo++] = '^';
					for (int t = 0; t < len; ++t) { if (mo > lim) { fits = false; break; } mdp[mo++] = class_to_char(fclass(ref0 + ref_i)); ref_i += 1; }
					mismatch += len;
				} else {
					in_x_run = false;
					if (m_len > 0) { co += dev_put_num(cg + co, m_len); cg[co++] = 'M'; m_len = 0; }
					co += dev_put_num(cg + co, len); cg[co++] = 'I';
					read_i += len;
					mismatch += len;
				}
			}
			if (co > lim || mo > lim) fits = false;  // the last run may have used the head room the tail below needs: host fall-back
			if (fits) {
				mo += dev_put_num(mdp + mo, md_eq);
				if (m_len > 0) { co += dev_put_num(cg + co, m_len); cg[co++] = 'M'; }
				if (trail > 0) {
					if (hard_clip == 1) { co += dev_put_num(cg + co, trail); cg[co++] = 'H'; }
					else if (silent_clip != 1) { co += dev_put_num(cg + co, trail); cg[co++] = 'S'; }
					o.qend = trail;
				}
			}
			o.identity = (float) match * 1.0f / (float) total;
			o.nm = mismatch;
			o.score_token = (float) read_i;
			o.position_offset = ref0;
			o.flags = ((fits && !odd_symbol) ? 1 : 0) | 2;
		}
	}
	}  // live
	o.cig_len = (uint16_t) co; o.md_len = (uint16_t) mo;
	// this workgroup's piece of the stream
	const uint32_t need = (live && (o.flags & 1)) ? (uint32_t) (co + mo) : 0u;
	uint32_t incl = need;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
	if (lane == 63) s_wave[wv] = incl;
	__syncthreads();
	uint32_t before = incl - need, total = 0;
#pragma unroll
	for (int w2 = 0; w2 < 4; ++w2) { if (w2 < wv) before += s_wave[w2]; total += s_wave[w2]; }
	if (threadIdx.x == 0) s_base = total ? atomicAdd(cursor, (unsigned long long) total) : 0ull;
	__syncthreads();
	const unsigned long long base = s_base;
	if (!live) return;
	if (need) {
		if (base + total > capacity) o.flags &= ~1;  // stream full: built on the host
		else {
			const unsigned long long off = base + before;
			o.cig_off = (uint32_t) off; o.md_off = (uint32_t) off + o.cig_len;
			for (int t = 0; t < co; ++t) bytes[off + t] = cg[t];
			for (int t = 0; t < mo; ++t) bytes[off + co + t] = mdp[t];
		}
	}
	out[j] = o;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Affine personality, one launch from the trace matrix to the strings: what affine_traceback_kernel + compact_runs_kernel +
// cigar_strings_kernel<true> do in three launches and two round trips through a strided runs scratch.
//   walk     SeqAn's single-trace, gaps-left traceback, step for step that of affine_traceback_kernel (one trace value, one move
//            per iteration; the two inner gap loops of the reference are the states `in_v` / `in_h`).  One lane per alignment, lane
//            = slot of the 64-way interleaved block.  The walk goes up the read in groups of kFinishRows rows: per group a lane
//            takes the trace words of those rows at the word of its current band column, the packed read word of the group
//            (eight symbols = eight rows) and the two window words under its diagonal in ONE batch of independent loads, then
//            consumes them.  The old walk made a dependent load per step (~150 round trips per alignment, now ~19).  A step whose
//            word is not the prefetched one (an indel carried the path over a column multiple of 8) loads directly: the result
//            never depends on a prefetch hit.
//   runs     never leave the chip: the walk emits them end -> start, so the CIGAR is written right to left into the lane's LDS
//            row, behind the trailing soft clip (QEnd = read length - end row is known before the walk).
//   strings  CIGAR, "!!!" as MD, NM, identity, QStart / QEnd, PositionOffset with the arithmetic of cigar_strings_kernel<true>;
//            the workgroup's strings leave as one piece of the compact byte stream (block prefix sum, one atomic on counters[0]).
//            A CIGAR is "valid" under the same condition as there: clip + runs take at most kCigarRow - 16 bytes (its check
//            before every run is monotone, so it amounts to the check behind the last one).
//   counters [0] cursor of the byte stream, [1] alignments left to the host (flag bit 0 clear).
// `records` is only read (rec[3] = end-cell flags of the 32-bit DP, rec[6] / rec[7] = end cell): the old kernels can still be run on
// the batch afterwards -- that is how the host serves the alignments counted in counters[1].
constexpr int kFinishRows = 8;   // rows per batch of loads == symbols per packed word

// entry k of eight registers (by value: a conditional between two array elements is one load from a selected address, which sends the array to scratch)
__device__ __forceinline__ uint32_t finish_sel8(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6, uint32_t w7, int k) {
	const uint32_t a0 = (k & 1) ? w1 : w0, a1 = (k & 1) ? w3 : w2, a2 = (k & 1) ? w5 : w4, a3 = (k & 1) ? w7 : w6;
	const uint32_t b0 = (k & 2) ? a1 : a0, b1 = (k & 2) ? a3 : a2;
	return (k & 4) ? b1 : b0;
}

template <bool NIBBLES>   // NIBBLES: the 4-bit trace of sw_affine_align_pk_kernel, else one trace byte per cell
__global__ __launch_bounds__(256) void affine_finish_kernel(int n, const uint32_t *__restrict__ dirs, const int32_t *__restrict__ records,
		const uint32_t *__restrict__ packed, const uint16_t *__restrict__ lens, int q, int CP, int RW, int FW, CigarDevOut *__restrict__ out,
		char *__restrict__ bytes, unsigned long long capacity, unsigned long long *__restrict__ counters) {
	__shared__ char s_rows[256 * kCigarRow];
	__shared__ uint32_t s_wave[4];
	__shared__ unsigned long long s_base;
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	const bool live = j < n;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	constexpr int lim = kCigarRow - 16;
	constexpr int WS = NIBBLES ? 3 : 2;   // band columns per trace word, as a shift
	const int DW = NIBBLES ? aff_nib_words(CP) : aff_dir_words(CP);
	char *row = s_rows + (size_t) threadIdx.x * kCigarRow;
	int pos = kCigarRow;   // the string grows downwards from the end of the row
	auto put_back = [&](int num, char tag) {
		row[--pos] = tag;
		unsigned u = (unsigned) num;
		do { row[--pos] = (char) ('0' + u % 10u); u /= 10u; } while (u);
	};
	bool fits = true;
	int h = 0, v = 0, flags = 0, len_v = 0;
	if (live) {
		const int32_t *rec = records + (size_t) j * 8;
		flags = rec[3]; h = rec[6]; v = rec[7];
		len_v = (int) lens[j];
	}
	const int qend = len_v - v;   // read length - (QStart + read characters of the alignment): the walk ends at row QStart
	if (live && qend > 0) put_back(qend, 'S');
	const int trail = kCigarRow - pos;
	const uint32_t *dp = dirs + (size_t) (j >> 6) * q * DW * kSlots + lane;
	const uint32_t *pk = packed + (size_t) (j >> 6) * (RW + FW) * kSlots + lane;
	int cur = -1, curlen = 0, total = 0, n_match = 0, n_mis = 0;
	bool done = !live, first = true, in_v = false, in_h = false;
	auto flush = [&]() {
		if (cur < 0) return;
		if (kCigarRow - pos - trail > lim) { fits = false; done = true; return; }   // already too long without this run and the clip
		put_back(curlen, cur == 1 ? 'M' : cur == 2 ? 'I' : 'D');
		total += cur == 1 ? curlen : 1;
	};
	auto emit = [&](int op) {
		if (op == cur) { ++curlen; return; }
		flush();
		cur = op; curlen = 1;
	};
	// the wave's first group: the highest end row of its lanes
	int gtop = (v - 1) >> 3;   // -1: nothing to walk
#pragma unroll
	for (int s = 1; s < 64; s <<= 1) gtop = max(gtop, __shfl_xor(gtop, s));
	for (int g = gtop; g >= 0; --g) {
		const int r0 = g * kFinishRows;
		const bool act = !done && v - 1 >= r0;   // (then v - 1 < r0 + kFinishRows: a lane enters a group from the one above, or starts in it)
		const int d0 = h - v;
		const int wi = min(max(d0 >> WS, 0), DW - 1);
		const int f0 = min(max((r0 + d0) >> 3, 0), FW - 1);
		uint32_t W[kFinishRows];
#pragma unroll
		for (int k = 0; k < kFinishRows; ++k) W[k] = (act && r0 + k <= v - 1) ? dp[((size_t) (r0 + k) * DW + wi) * kSlots] : 0u;
		const uint32_t rdw = act ? pk[(size_t) g * kSlots] : 0u;
		const uint32_t fw0 = act ? pk[(size_t) (RW + f0) * kSlots] : 0u;
		const uint32_t fw1 = (act && f0 + 1 < FW) ? pk[(size_t) (RW + f0 + 1) * kSlots] : 0u;
		// the common case in one go: the rows of this group the path crosses diagonally, from its current row down, all in the prefetched
		// word -- one diagonal test per row, the match count by a byte-wise compare of the group's read word with the window under it.
		// (Outside a gap a cell with the diagonal bit is a diagonal step whatever else it holds.  The first cell of a walk goes through the
		// loop below for its corrections -- except with the 4-bit trace and no end-cell flags, where they leave a diagonal cell as it is:
		// such a cell has neither maximum bit.)  This is what makes the walk a matter of memory, not of ~100 instructions per step.
		if (act && (!first || (NIBBLES && flags == 0)) && !in_v && !in_h) {
			const int kc = v - 1 - r0;
			if (d0 >= 0 && d0 < CP && (d0 >> WS) == wi && ((r0 + d0) >> 3) == f0 && f0 + 1 < FW) {
				const int sh = NIBBLES ? 4 * (d0 & 7) : 8 * (d0 & 3);
				uint32_t m = 0;
#pragma unroll
				for (int k = 0; k < kFinishRows; ++k) m |= (NIBBLES ? (uint32_t) (((W[k] >> sh) & 0xCu) == 4u) : ((W[k] >> sh) & 1u)) << k;
				const uint32_t stop = ~m & ((2u << kc) - 1u);   // rows at or below the current one that are no diagonal step
				const int lo = stop ? 32 - __clz((int) stop) : 0;   // the run: rows lo .. kc
				const int run = kc + 1 - lo;
				if (run > 0) {
					auto spread = [](uint32_t x) -> unsigned long long { return (unsigned long long) (x & 0x0F0F0F0Fu) | ((unsigned long long) ((x >> 4) & 0x0F0F0F0Fu) << 32); };   // byte k = symbol k
					const unsigned long long ones = 0x0101010101010101ull, RB = spread(rdw), A = spread(fw0), B = spread(fw1);
					const int o = (r0 + d0) & 7;
					const unsigned long long WB = o ? (A >> (8 * o)) | (B << (64 - 8 * o)) : A;   // window symbols under rows 0..7
					const unsigned long long differ = (((RB ^ WB) + 0x0F0F0F0F0F0F0F0Full) >> 4) & ones;
					const unsigned long long odd = (RB >> 2) & (~RB | (RB >> 1)) & ones;         // read classes 4, 6, 7 match nothing
					const unsigned long long upto = kc == 7 ? ~0ull : (1ull << (8 * (kc + 1))) - 1ull;
					const int mis = __popcll((differ | odd) & upto & ~((1ull << (8 * lo)) - 1ull));
					n_mis += mis; n_match += run - mis;
					if (cur != 1) { flush(); cur = 1; curlen = 0; }
					curlen += run; h -= run; v -= run;
					first = false;
				}
			}
		}
		while (!done && v - 1 >= r0) {
			// the trace value of cell (h, v); v > 0 here
			const int d = h - v;
			uint32_t tv = 0u;
			if (h > 0 && d >= 0 && d < CP) {
				const int w = d >> WS;
				const uint32_t word = (w == wi) ? finish_sel8(W[0], W[1], W[2], W[3], W[4], W[5], W[6], W[7], v - 1 - r0) : dp[((size_t) (v - 1) * DW + w) * kSlots];
				tv = NIBBLES ? aff_trace_from_nibble((word >> (4 * (d & 7))) & 15u, d, CP) : (word >> (8 * (d & 3))) & 0xFFu;
			}
			if (first) {
				first = false;
				// _correctTraceValue (dp_algorithm_impl.h:1233-1250)
				if (flags & 1) tv = (tv & ~(uint32_t) kTDiag) | (uint32_t) kTMaxV;
				else if (flags & 2) tv = (tv & ~(uint32_t) kTDiag) | (uint32_t) kTMaxH;
				// _retrieveInitialTraceDirection, PreferGapsAtEnd (dp_traceback_impl.h:452-468)
				if (tv & kTMaxV) tv &= (uint32_t) (kTVert | kTVertOpen | kTMaxV);
				else if (tv & kTMaxH) tv &= (uint32_t) (kTHori | kTHoriOpen | kTMaxH);
			}
			if (!in_v && !in_h) {
				if (h <= 0 || tv == 0u) { done = true; break; }
				if (tv & kTDiag) {
					emit(1);
					const int jr = (v - 1) & 7, jf = (h - 1) & 7, fi = (h - 1) >> 3;
					const uint32_t fx = (fi == f0) ? fw0 : (fi == f0 + 1) ? fw1 : pk[(size_t) (RW + fi) * kSlots];
					const uint32_t rc = (rdw >> (4 * ((jr & 3) * 2 + (jr >> 2)))) & 15u, fc = (fx >> (4 * ((jf & 3) * 2 + (jf >> 2)))) & 15u;
					if (rc == fc && rc <= 5u && rc != 4u) ++n_match; else ++n_mis;
					--h; --v;
					continue;
				}
				if ((tv & kTMaxV) && (tv & kTVert)) in_v = true;
				else if ((tv & kTMaxV) && (tv & kTVertOpen)) { emit(2); --v; continue; }
				else if ((tv & kTMaxH) && (tv & kTHori)) in_h = true;
				else if ((tv & kTMaxH) && (tv & kTHoriOpen)) { emit(3); --h; continue; }
				else { done = true; break; }
			}
			// inside a gap: one step per trace value, the last one when the gap was opened here (or at row / column 1)
			if (in_v) { in_v = (!(tv & kTVertOpen) || (tv & kTVert)) && v != 1; emit(2); --v; }
			else { in_h = (!(tv & kTHoriOpen) || (tv & kTHori)) && h != 1; emit(3); --h; }
		}
	}
	int co = 0;
	if (live) {
		if (fits) flush();
		int lead = 0;
		if (v > 0) { lead = 2; for (int t = v; t >= 10; t /= 10) ++lead; }
		if (kCigarRow - pos - trail + lead > lim) fits = false;
		if (fits && v > 0) put_back(v, 'S');
		co = kCigarRow - pos;
	}
	constexpr int mo = 3;   // EndToEndAffine never touches pBuffer2: the record carries AlignmentBuffer's "!!!" (AlignmentBuffer.cpp:109)
	// this workgroup's piece of the stream
	const uint32_t need = (live && fits) ? (uint32_t) (co + mo) : 0u;
	uint32_t incl = need;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
	if (lane == 63) s_wave[wv] = incl;
	__syncthreads();
	uint32_t before = incl - need, total_b = 0;
#pragma unroll
	for (int w2 = 0; w2 < 4; ++w2) { if (w2 < wv) before += s_wave[w2]; total_b += s_wave[w2]; }
	if (threadIdx.x == 0) s_base = total_b ? atomicAdd(&counters[0], (unsigned long long) total_b) : 0ull;
	__syncthreads();
	const unsigned long long base = s_base;
	if (!live) return;
	uint32_t cig_off = 0;
	if (need) {
		if (base + total_b > capacity) fits = false;  // stream full: built on the host
		else {
			const unsigned long long off = base + before;
			cig_off = (uint32_t) off;
			const char *cg = row + pos;
			for (int t = 0; t < co; ++t) bytes[off + t] = cg[t];
			for (int t = 0; t < mo; ++t) bytes[off + co + t] = '!';
		}
	}
	if (!fits) atomicAdd(&counters[1], 1ull);
	CigarDevOut *o = out + j;
	o->cig_off = cig_off; o->md_off = fits ? cig_off + (uint32_t) co : 0u;
	o->cig_len = (uint16_t) co; o->md_len = (uint16_t) mo;
	o->position_offset = h; o->qstart = v; o->qend = qend; o->nm = n_mis;
	o->identity = (float) n_match * 1.0f / (float) total;
	o->score_token = 0.f;
	o->flags = (fits ? 1 : 0) | 2;
}

}  // namespace ngm
