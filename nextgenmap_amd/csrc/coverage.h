// coverage.h -- the host-only parts of `ngm-hip --coverage` (csrc/coverage.cpp, csrc/coverage_device.h): the walk over a CIGAR text that yields
// the reference blocks an alignment covers, the validator of what ngm_coverage_add is given, the layout of the counter array, and the
// serialiser of the bedGraph lines (the host twin of the text kernels).  Compiles with plain g++ (tests/cpp/coverage_driver.cpp); the
// functions marked NGM_COV_HD are the ones the kernels run as well.
//
// The definition: an alignment covers the reference bases under its M, = and X operations (samtools depth's default); D and N advance the
// position without covering; I, S, H and P do neither; what would lie past the contig's last base is clipped.  A line is
// contig \t start \t end \t depth \n (start 0-based, end exclusive, depth > 0), one per maximal run of equal depth inside one contig.
//
// The counter array: one int32 per base of every contig plus one trailing slot per contig; contig c starts at the sum of (len_k + 1) over
// k < c.  A block [begin, end) adds +1 at begin and -1 at end, both inside its own contig's slots (end <= len_c: the trailing slot at most),
// so a plain inclusive scan over the whole array is 0 again at every contig's trailing slot and needs no restart per contig -- and a run
// never crosses a contig boundary, because a slot of depth 0 lies between any two contigs.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NGM_COV_HD __host__ __device__
#else
#define NGM_COV_HD
#endif

namespace ngm {
namespace cov {

constexpr uint32_t kMaxOpLen = 1u << 28;   // an operation's length stays below this (the 28 bits a BAM record has for it)

// why an alignment is refused
enum { kOk = 0, kBadRef = 1, kBadPos = 2, kBadOp = 3, kOverflow = 4, kNoNumber = 5, kNoOp = 6 };

// 0: covers (M = X), 1: advances only (D N), 2: neither (I S H P), -1: unknown
NGM_COV_HD inline int op_kind(char ch) {
	switch (ch) {
	case 'M': case '=': case 'X': return 0;
	case 'D': case 'N': return 1;
	case 'I': case 'S': case 'H': case 'P': return 2;
	default: return -1;
	}
}

// the covered blocks of one alignment, clipped to [0, contig_len): f(begin, end), begin < end, ascending.  Neighbouring covering operations
// (also across an I, S, H or P) form one block.  Numbers saturate at kMaxOpLen and unknown operations do nothing: text the validator has
// not seen (the mapper's own) can at worst cover a clipped block of its own contig.
template <typename F>
NGM_COV_HD inline void walk_cigar(int64_t pos0, const char *cigar, uint32_t n, int64_t contig_len, F f) {
	int64_t at = pos0, b = pos0, e = pos0;   // [b, e): the block being gathered
	uint64_t num = 0;
	auto flush = [&]() {
		const int64_t lo = b < 0 ? 0 : b, hi = e < contig_len ? e : contig_len;
		if (lo < hi) f(lo, hi);
	};
	for (uint32_t i = 0; i < n; ++i) {
		const char ch = cigar[i];
		if (ch >= '0' && ch <= '9') { num = num * 10u + (uint64_t) (ch - '0'); if (num > kMaxOpLen) num = kMaxOpLen; continue; }
		const int kind = op_kind(ch);
		if (kind == 0) {
			if (e != at) { flush(); b = at; }
			at += (int64_t) num;
			e = at;
		} else if (kind == 1) at += (int64_t) num;
		num = 0;
	}
	flush();
}

// the checks of ngm_coverage_add: kOk, or why not
NGM_COV_HD inline int check_alignment(int32_t ref_id, int32_t pos0, const char *cigar, uint32_t n, int n_ref) {
	if (ref_id < 0 || ref_id >= n_ref) return kBadRef;
	if (pos0 < 0) return kBadPos;
	uint64_t num = 0;
	bool digits = false;
	for (uint32_t i = 0; i < n; ++i) {
		const char ch = cigar[i];
		if (ch >= '0' && ch <= '9') {
			num = num * 10u + (uint64_t) (ch - '0');
			if (num >= kMaxOpLen) return kOverflow;
			digits = true;
			continue;
		}
		if (op_kind(ch) < 0) return kBadOp;
		if (!digits) return kNoNumber;
		num = 0;
		digits = false;
	}
	return digits ? kNoOp : kOk;
}

inline const char *why(int code) {
	switch (code) {
	case kBadRef: return "its ref_id is not in [0, n_ref)";
	case kBadPos: return "its position is negative";
	case kBadOp: return "its CIGAR has an unknown operation character";
	case kOverflow: return "a number in its CIGAR overflows 2^28";
	case kNoNumber: return "its CIGAR has an operation without a number";
	case kNoOp: return "its CIGAR ends in a number without an operation";
	default: return "ok";
	}
}

// where contig c starts in the counter array: offsets[n_ref] is the array's size
inline std::vector<uint64_t> contig_offsets(const uint32_t *ref_len, int n_ref) {
	std::vector<uint64_t> off((size_t) n_ref + 1, 0);
	for (int c = 0; c < n_ref; ++c) off[(size_t) c + 1] = off[c] + (uint64_t) ref_len[c] + 1u;
	return off;
}

// the contig whose slots hold array offset g (g < off[n_ref]): the last c with off[c] <= g
NGM_COV_HD inline int contig_of(const uint64_t *off, int n_ref, uint64_t g) {
	int lo = 0, hi = n_ref - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (off[mid] <= g) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// host: one alignment into a counter array on the host (the +1 / -1 pairs the add kernel issues)
inline void add_host(int32_t *counters, const uint64_t *off, const uint32_t *ref_len, int32_t ref_id, int32_t pos0, const char *cigar, uint32_t n) {
	int32_t *base = counters + off[ref_id];
	walk_cigar(pos0, cigar, n, (int64_t) ref_len[ref_id], [&](int64_t b, int64_t e) { base[b] += 1; base[e] -= 1; });
}

inline void put_u64(std::string &s, unsigned long long v) {
	char b[24];
	int i = 24;
	do { b[--i] = (char) ('0' + (int) (v % 10ull)); v /= 10ull; } while (v);
	s.append(b + i, (size_t) (24 - i));
}

// host: the file of a counter array.  totals: covered bases (the sum of (end - start) * depth), runs, when asked for
inline void serialise(const int32_t *counters, const uint64_t *off, int n_ref, const char *const *ref_name, std::string &out, uint64_t *covered = nullptr, uint64_t *runs = nullptr) {
	uint64_t n_cov = 0, n_runs = 0;
	int64_t depth = 0;
	for (int c = 0; c < n_ref; ++c) {
		const uint64_t len = off[(size_t) c + 1] - off[c] - 1;
		uint64_t start = 0;
		int64_t open = 0;   // depth of the run that began at start
		for (uint64_t p = 0; p <= len; ++p) {   // (the trailing slot takes the depth back to 0 and closes the last run)
			depth += counters[off[c] + p];
			if (depth == open) continue;
			if (open > 0) {
				out += ref_name[c]; out.push_back('\t'); put_u64(out, start); out.push_back('\t'); put_u64(out, p); out.push_back('\t'); put_u64(out, (unsigned long long) open); out.push_back('\n');
				n_cov += (p - start) * (uint64_t) open;
				++n_runs;
			}
			start = p;
			open = depth;
		}
	}
	if (covered) *covered = n_cov;
	if (runs) *runs = n_runs;
}

}  // namespace cov
}  // namespace ngm
