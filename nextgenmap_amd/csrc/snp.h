// snp.h -- the host-only parts of `ngm-hip --snp` (csrc/snp.cpp, csrc/snp_device.h): the walk over a CIGAR text that yields the aligned
// segments of a record with their read offsets, the two checks ngm_snp_add makes on top of coverage.h's, the packed reference, the call
// rule, and the serialiser of the VCF (the host twin of the add, flag and text kernels).  Compiles with plain g++
// (tests/cpp/snp_driver.cpp); the functions marked NGM_COV_HD are the ones the kernels run as well.
//
// The definition ("--snp"): depth is --coverage's depth.  A record walks its CIGAR over its sequence as the SAM record
// prints it (I and S consume read bases, H and P nothing); an M, = or X column at contig position p with read base b and reference base r
// adds 1 to alt[p][b] when p is inside the contig, r and b are one of ACGT (the reference's case folded), b != r, and the record has no
// quality string or the column's Phred quality is at least Q.  p is a call when depth >= max(1, N) and (double) n >= F * (double) depth
// for the alternative a with the largest count n > 0 (ties: the first of A, C, G, T).
//
// The counters: the difference array of coverage.h (one int32 per base plus a trailing slot per contig) and, beside it, three uint32 per
// slot.  A mismatching base b over a reference base r (classes A0 C1 G2 T3) lands in slot (b - r - 1) & 3 of the three: b != r leaves
// exactly the values 0, 1, 2, so the reference base itself needs no counter and a base costs 4 + 12 = 16 bytes.  Four counters indexed by
// b alone would need a depth of less than 32 bits to stay within 16 bytes.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "coverage.h"

namespace ngm {
namespace snp {

// further reasons ngm_snp_add refuses an alignment for (after coverage.h's)
enum { kSeqLength = 16, kQualLength = 17, kBadOffsets = 18 };

inline const char *why(int code) {
	switch (code) {
	case kSeqLength: return "its sequence is shorter or longer than the read bases its CIGAR consumes";
	case kQualLength: return "its quality text has another length than its sequence";
	case kBadOffsets: return "its offsets do not ascend";
	default: return cov::why(code);
	}
}

// the 4-bit classes of the packed reference (refindex.h): A0 C1 G2 T3, any other letter 4, N 5; case folded
NGM_COV_HD inline uint32_t ref_class_of(char ch) {
	switch (ch) {
	case 'A': case 'a': return 0u;
	case 'C': case 'c': return 1u;
	case 'G': case 'g': return 2u;
	case 'T': case 't': return 3u;
	case 'N': case 'n': return 5u;
	default: return 4u;
	}
}
// a read base as the record prints it: only the four upper-case letters vote
NGM_COV_HD inline uint32_t read_class_of(char ch) { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u; }
NGM_COV_HD inline uint32_t packed_class(const uint32_t *genome, uint64_t p) { return (genome[p >> 3] >> (4u * (uint32_t) (p & 7u))) & 15u; }
NGM_COV_HD inline uint32_t alt_slot(uint32_t b, uint32_t r) { return (b - r - 1u) & 3u; }   // b != r, both in 0..3: 0, 1 or 2

// the contigs one after the other without gaps, 8 bases per dword: start[c] is the base offset of contig c, start[n_ref] the total
inline std::vector<uint32_t> pack_reference(const char *const *ref_seq, const uint32_t *ref_len, int n_ref, std::vector<uint64_t> &start) {
	start.assign((size_t) n_ref + 1, 0);
	for (int c = 0; c < n_ref; ++c) start[(size_t) c + 1] = start[c] + ref_len[c];
	std::vector<uint32_t> words((size_t) ((start[n_ref] + 7) / 8) + 1, 0u);
	for (int c = 0; c < n_ref; ++c)
		for (uint64_t i = 0; i < ref_len[c]; ++i) {
			const uint64_t p = start[c] + i;
			words[(size_t) (p >> 3)] |= ref_class_of(ref_seq[c][i]) << (4u * (uint32_t) (p & 7u));
		}
	return words;
}

// the aligned segments of one record, clipped to [0, contig_len): f(begin, end, read offset of begin), begin < end.  Numbers saturate as
// in cov::walk_cigar; the read offset counts the bases of M, =, X, I and S in front.
template <typename F>
NGM_COV_HD inline void walk_segments(int64_t pos0, const char *cigar, uint32_t n, int64_t contig_len, F f) {
	int64_t at = pos0;
	uint64_t ri = 0, num = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const char ch = cigar[i];
		if (ch >= '0' && ch <= '9') { num = num * 10u + (uint64_t) (ch - '0'); if (num > cov::kMaxOpLen) num = cov::kMaxOpLen; continue; }
		const int kind = cov::op_kind(ch);
		if (kind == 0) {
			const int64_t lo = at < 0 ? 0 : at, hi = at + (int64_t) num < contig_len ? at + (int64_t) num : contig_len;
			if (lo < hi) f(lo, hi, ri + (uint64_t) (lo - at));
			at += (int64_t) num;
			ri += num;
		} else if (kind == 1) at += (int64_t) num;
		else if (ch == 'I' || ch == 'S') ri += num;
		num = 0;
	}
}

// the read bases a (validated) CIGAR consumes
NGM_COV_HD inline uint64_t read_bases_of(const char *cigar, uint32_t n) {
	uint64_t ri = 0, num = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const char ch = cigar[i];
		if (ch >= '0' && ch <= '9') { num = num * 10u + (uint64_t) (ch - '0'); if (num > cov::kMaxOpLen) num = cov::kMaxOpLen; continue; }
		if (cov::op_kind(ch) == 0 || ch == 'I' || ch == 'S') ri += num;
		num = 0;
	}
	return ri;
}

// the checks of ngm_snp_add: coverage.h's, then the sequence's length (a quality text shares the sequence's offsets, so its length is
// checked by the caller against the whole text)
inline int check_alignment(int32_t ref_id, int32_t pos0, const char *cigar, uint32_t n, int n_ref, uint64_t seq_len) {
	const int code = cov::check_alignment(ref_id, pos0, cigar, n, n_ref);
	if (code != cov::kOk) return code;
	return read_bases_of(cigar, n) == seq_len ? (int) cov::kOk : (int) kSeqLength;
}

// the thresholds: min_cov N, min_frac F, min_qual Q
struct Rule { uint32_t min_cov; double min_frac; int min_qual; };

// the call of one base: counters k[3] over reference class r (0..3); the alternative's class into *alt, its count returned (0: no call)
NGM_COV_HD inline uint32_t call_of(int64_t depth, uint32_t r, const uint32_t *k, const Rule &rule, uint32_t *alt) {
	uint32_t best = 0, best_b = 0;
	for (uint32_t b = 0; b < 4u; ++b) {
		if (b == r) continue;
		const uint32_t n = k[alt_slot(b, r)];
		if (n > best) { best = n; best_b = b; }
	}
	if (best == 0) return 0;
	const int64_t need = rule.min_cov > 1u ? (int64_t) rule.min_cov : 1;
	if (depth < need) return 0;
	if (!((double) best >= rule.min_frac * (double) depth)) return 0;
	*alt = best_b;
	return best;
}

// host: one record into counter arrays on the host (what the add kernel issues); returns the mismatching bases counted
inline uint64_t add_host(int32_t *diff, uint32_t *alt, const uint64_t *off, const uint32_t *ref_len, const uint32_t *genome, const uint64_t *start, int min_qual,
		int32_t ref_id, int32_t pos0, const char *cigar, uint32_t n, const char *seq, const char *qual) {
	cov::add_host(diff, off, ref_len, ref_id, pos0, cigar, n);
	uint64_t counted = 0;
	walk_segments(pos0, cigar, n, (int64_t) ref_len[ref_id], [&](int64_t b, int64_t e, uint64_t ri) {
		for (int64_t p = b; p < e; ++p, ++ri) {
			const uint32_t r = packed_class(genome, start[ref_id] + (uint64_t) p), c = read_class_of(seq[ri]);
			if (r > 3u || c > 3u || c == r) continue;
			if (qual && (int) (unsigned char) qual[ri] - 33 < min_qual) continue;
			alt[3u * (off[ref_id] + (uint64_t) p) + alt_slot(c, r)] += 1u;
			++counted;
		}
	});
	return counted;
}

// the header: min_frac_text is the option's text
inline std::string header(int n_ref, const char *const *ref_name, const uint32_t *ref_len, const Rule &rule, const char *min_frac_text) {
	std::string h = "##fileformat=VCFv4.2\n##source=ngm-hip --snp (min-cov ";
	cov::put_u64(h, rule.min_cov); h += ", min-frac "; h += min_frac_text; h += ", min-qual "; cov::put_u64(h, (unsigned long long) rule.min_qual); h += ")\n";
	for (int c = 0; c < n_ref; ++c) { h += "##contig=<ID="; h += ref_name[c]; h += ",length="; cov::put_u64(h, ref_len[c]); h += ">\n"; }
	h += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"records covering the base\">\n";
	h += "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"records with the ALT base at quality >= "; cov::put_u64(h, (unsigned long long) rule.min_qual); h += "\">\n";
	h += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
	return h;
}

// host: the lines of the counter arrays (no header).  totals: calls, covered bases (the sum of the depths), when asked for
inline void serialise(const int32_t *diff, const uint32_t *alt, const uint64_t *off, int n_ref, const char *const *ref_name, const uint32_t *genome, const uint64_t *start,
		const Rule &rule, std::string &out, uint64_t *calls = nullptr, uint64_t *covered = nullptr) {
	uint64_t n_calls = 0, n_cov = 0;
	int64_t depth = 0;
	for (int c = 0; c < n_ref; ++c) {
		const uint64_t len = off[(size_t) c + 1] - off[c] - 1;
		for (uint64_t p = 0; p <= len; ++p) {
			depth += diff[off[c] + p];
			if (p == len) break;   // (the trailing slot only takes the depth back to 0)
			n_cov += (uint64_t) depth;
			const uint32_t r = packed_class(genome, start[c] + p);
			if (r > 3u) continue;
			uint32_t a = 0;
			const uint32_t n = call_of(depth, r, alt + 3u * (off[c] + p), rule, &a);
			if (!n) continue;
			out += ref_name[c]; out.push_back('\t'); cov::put_u64(out, p + 1); out += "\t.\t"; out.push_back("ACGT"[r]); out.push_back('\t'); out.push_back("ACGT"[a]);
			out += "\t.\tPASS\tDP="; cov::put_u64(out, (unsigned long long) depth); out += ";AO="; cov::put_u64(out, n); out.push_back('\n');
			++n_calls;
		}
	}
	if (calls) *calls = n_calls;
	if (covered) *covered = n_cov;
}

}  // namespace snp
}  // namespace ngm
