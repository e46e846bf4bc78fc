// methyl.h -- the host-only parts of `ngm-hip --bs-mapping --methyl` (csrc/methyl.cpp, csrc/methyl_device.h): the walk of one record over
// the counters (add_record: the add kernel runs this very function, with atomics for a sink), the context of a site, the line of a site
// (the host twin of the text kernels) and the serialiser of the file.  Compiles with plain g++ (tests/cpp/methyl_driver.cpp); the functions
// marked NGM_COV_HD are the ones the kernels run as well.  The per-alignment checks are ngm_snp_add's (snp::check_alignment).
//
// The definition ("--methyl").  The records that count are --coverage's.  A record is top when the ZS:Z tag it gets begins
// with '+' and bottom when it begins with '-': bottom = (flag 0x10 set) XOR (paired run and flag 0x80 set).  A record walks its CIGAR over
// its sequence as the SAM record prints it (snp::walk_segments).  An M, = or X column at contig position p inside the contig with printed
// read base b counts when the record has no quality string or the column's Phred quality is at least Q: a top record over a reference C
// (case folded) adds 1 to meth[p] when b is C and 1 to unmeth[p] when b is T; a bottom record over a reference G adds 1 to meth[p] when b
// is G and 1 to unmeth[p] when b is A.  Anything else adds nothing.
//
// The counters: one pair of uint32 (meth, unmeth) per base of the reference, the contigs one behind the other without a gap -- a base is C,
// G or neither, so one pair serves both strands and a base costs 8 bytes.  There is no depth array.
//
// A site is a reference C (strand +) or G (strand -).  Its context: for a C, n1 = ref[p + 1] and n2 = ref[p + 2]; for a G, n1 = the
// complement of ref[p - 1] and n2 = the complement of ref[p - 2]; a neighbour outside the same contig, or not one of ACGT, is N.  n1 == G:
// CG; n1 == N: CN; otherwise n2 == G: CHG, n2 == N: CHN, else CHH.  A site is a line of the file when meth + unmeth >= max(1, N) and its
// context is selected: "name \t p + 1 \t strand \t meth \t unmeth \t context \t C n1 n2 \n", in reference order, no header.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "snp.h"

namespace ngm {
namespace met {

constexpr int kDefaultMinQual = 5;    // MethylDackel's -p
constexpr int kDefaultMinDepth = 1;

// the contexts, and the bit each has in a selection
enum { kCG = 0, kCHG = 1, kCHH = 2, kCN = 3, kCHN = 4 };
constexpr uint32_t kSelectAll = 31u;

// the selection a --methyl-context name stands for; 0: not one of the four
inline uint32_t selection_of(const char *name) {
	if (!strcmp(name, "all")) return kSelectAll;
	if (!strcmp(name, "CpG")) return 1u << kCG;
	if (!strcmp(name, "CHG")) return 1u << kCHG;
	if (!strcmp(name, "CHH")) return 1u << kCHH;
	return 0u;
}

NGM_COV_HD inline const char *context_name(int ctx) { return ctx == kCG ? "CG" : ctx == kCHG ? "CHG" : ctx == kCHH ? "CHH" : ctx == kCN ? "CN" : "CHN"; }

// where the records add: pointers into host or device memory
struct Layout {
	const uint64_t *off;       // [n_ref + 1] a contig's first pair in the counters (the sum of the lengths in front of it)
	const uint32_t *genome;    // 4-bit classes, 8 per dword (snp.h)
	const uint64_t *start;     // [n_ref] base offset of a contig in genome
	int n_ref, min_qual;
};

// the counters' offsets: off[n_ref] pairs in all
inline std::vector<uint64_t> pair_offsets(const uint32_t *ref_len, int n_ref) {
	std::vector<uint64_t> off((size_t) n_ref + 1, 0);
	for (int c = 0; c < n_ref; ++c) off[(size_t) c + 1] = off[c] + (uint64_t) ref_len[c];
	return off;
}

// a record on the host
struct HostRec {
	int contig; int64_t pos0; const char *cigar; uint32_t cigar_len, seq_len;
	const char *seq, *qual;
	char base(uint32_t i) const { return seq[i]; }
	bool qual_ok(uint32_t i, int min_qual) const { return !qual || (int) (unsigned char) qual[i] - 33 >= min_qual; }
};

// One record into the counters.  sink.add(i): +1 on counter i (2 * pair: meth, 2 * pair + 1: unmeth).  stat[0]: the methylated calls the
// record made, stat[1]: the unmethylated ones.
template <typename RecT, typename Sink>
NGM_COV_HD inline void add_record(const Layout &L, const RecT &rec, bool bottom, Sink &sink, uint32_t stat[2]) {
	stat[0] = stat[1] = 0;
	const int c = rec.contig;
	if (c < 0 || c >= L.n_ref || rec.pos0 < 0) return;   // (never from the validated arrays; the mapper's records have a contig)
	const uint64_t base = L.off[c], g0 = L.start[c];
	const int64_t len = (int64_t) (L.off[c + 1] - base);
	const uint32_t site = bottom ? 2u : 1u, converted = bottom ? 0u : 3u;   // a G read as G or A, a C read as C or T
	uint64_t w_at = ~0ull;
	uint32_t w = 0, meth = 0, unmeth = 0;
	snp::walk_segments(rec.pos0, rec.cigar, rec.cigar_len, len, [&](int64_t b, int64_t e, uint64_t ri) {
		for (int64_t p = b; p < e && ri < (uint64_t) rec.seq_len; ++p, ++ri) {   // (a validated record never runs out of bases)
			const uint64_t g = g0 + (uint64_t) p;
			if ((g >> 3) != w_at) { w_at = g >> 3; w = L.genome[w_at]; }   // the reference a dword (8 bases) at a time
			if (((w >> (4u * (uint32_t) (g & 7u))) & 15u) != site) continue;
			const uint32_t r = snp::read_class_of(rec.base((uint32_t) ri));
			if (r != site && r != converted) continue;
			if (!rec.qual_ok((uint32_t) ri, L.min_qual)) continue;
			if (r == site) { sink.add(2u * (base + (uint64_t) p)); ++meth; }
			else { sink.add(2u * (base + (uint64_t) p) + 1u); ++unmeth; }
		}
	});
	stat[0] = meth; stat[1] = unmeth;
}

// the sink of the host twin
struct HostSink {
	uint32_t *cnt;
	void add(uint64_t i) { cnt[i] += 1u; }
};

// ---- a site ------------------------------------------------------------------------------------------------------------------------
// the class of a neighbour as the site's strand reads it: 0..3, or 4 for N (outside the contig, or not one of ACGT)
NGM_COV_HD inline uint32_t neighbour(const uint32_t *genome, uint64_t g0, uint64_t len, int64_t p, bool minus) {
	if (p < 0 || (uint64_t) p >= len) return 4u;
	const uint32_t cls = snp::packed_class(genome, g0 + (uint64_t) p);
	return cls > 3u ? 4u : minus ? 3u - cls : cls;
}

// the context of the site of class cls (1: C, 2: G) at position p of a contig of len bases that begins at g0 of the packed reference;
// n[0], n[1]: the two neighbours' classes (4: N)
NGM_COV_HD inline int context_of(const uint32_t *genome, uint64_t g0, uint64_t len, uint64_t p, uint32_t cls, uint32_t n[2]) {
	const bool minus = cls == 2u;
	n[0] = neighbour(genome, g0, len, minus ? (int64_t) p - 1 : (int64_t) p + 1, minus);
	n[1] = neighbour(genome, g0, len, minus ? (int64_t) p - 2 : (int64_t) p + 2, minus);
	if (n[0] == 2u) return kCG;
	if (n[0] == 4u) return kCN;
	return n[1] == 2u ? kCHG : n[1] == 4u ? kCHN : kCHH;
}

// is the site with these counters a line: the depth rule and the selection
NGM_COV_HD inline bool is_line(uint32_t meth, uint32_t unmeth, int ctx, uint32_t min_depth, uint32_t selection) {
	const uint64_t depth = (uint64_t) meth + unmeth;
	return depth >= (min_depth > 1u ? (uint64_t) min_depth : 1ull) && ((selection >> ctx) & 1u);
}

// host: the file of a counter array, and the six sums -- meth and unmeth over all sites of context CG, CHG and CHH, whatever is selected
inline void serialise(const uint32_t *cnt, const uint64_t *off, int n_ref, const char *const *ref_name, const uint32_t *genome, const uint64_t *start, uint32_t min_depth,
		uint32_t selection, std::string &out, uint64_t *lines = nullptr, uint64_t sums[6] = nullptr) {
	uint64_t n_lines = 0, six[6] = {0, 0, 0, 0, 0, 0};
	for (int c = 0; c < n_ref; ++c) {
		const uint64_t len = off[(size_t) c + 1] - off[c];
		for (uint64_t p = 0; p < len; ++p) {
			const uint32_t cls = snp::packed_class(genome, start[c] + p);
			if (cls != 1u && cls != 2u) continue;
			const uint32_t meth = cnt[2u * (off[c] + p)], unmeth = cnt[2u * (off[c] + p) + 1u];
			uint32_t n[2];
			const int ctx = context_of(genome, start[c], len, p, cls, n);
			if (ctx <= kCHH) { six[2 * ctx] += meth; six[2 * ctx + 1] += unmeth; }
			if (!is_line(meth, unmeth, ctx, min_depth, selection)) continue;
			out += ref_name[c]; out.push_back('\t'); cov::put_u64(out, p + 1); out.push_back('\t'); out.push_back(cls == 1u ? '+' : '-'); out.push_back('\t');
			cov::put_u64(out, meth); out.push_back('\t'); cov::put_u64(out, unmeth); out.push_back('\t'); out += context_name(ctx);
			out.push_back('\t'); out.push_back('C'); out.push_back("ACGTN"[n[0]]); out.push_back("ACGTN"[n[1]]); out.push_back('\n');
			++n_lines;
		}
	}
	if (lines) *lines = n_lines;
	if (sums) for (int k = 0; k < 6; ++k) sums[k] = six[k];
}

}  // namespace met
}  // namespace ngm
