// count.h -- the host-only parts of `ngm-hip --count` (csrc/count.cpp, csrc/count_device.h): the reader of the BED file with its refusals,
// the tables a record finds its counters and its regions with, the walk of one record over them (add_record: the add kernel runs this very
// function, with atomics for a sink), the sums of one region (the host twin of the reduce kernel) and the serialiser of the file.  Compiles
// with plain g++ (tests/cpp/count_driver.cpp); the functions marked NGM_COV_HD are the ones the kernels run as well.
//
// The definition ("--count").  The records that count are --coverage's and --snp's; a record is forward when its flag bit
// 0x10 is clear and reverse when it is set.  A record walks its CIGAR over its sequence as the SAM record prints it (snp::walk_segments).
// An M, = or X column at contig position p with read base b is eligible when p is inside the contig, the case-folded reference base is T
// (forward record) or A (reverse record), b is one of ACGT, and the record has no quality string or the column's Phred quality is at least
// Q.  An eligible column adds 1 to cov[p], and 1 to conv[p] when b is C (forward) or G (reverse).  A region of strand + takes forward
// records, - reverse records, . both; reads[R] counts the records it takes that have an M / = / X column inside [start, end), tc_reads[R]
// those of them with an eligible column inside the region that is a conversion.  At the finish a region sums cov and conv over its
// positions whose reference base is T (+), A (-) or either (.) and that are not in the mask; t_bases counts those positions, masked the
// ones the mask took away.  tc_reads is taken when the record is added and does not know the mask.
//
// The counters: only bases that some region covers have any.  The regions of a contig are merged into disjoint intervals (touching ones
// too); interval k holds slots slot[k] .. slot[k] + (end[k] - start[k]), two uint32 (cov, conv) per slot -- a reference base is T, A or
// neither, so one pair serves both strands.  A position finds its slot by binary search over its contig's intervals.  The regions are
// also kept sorted by (contig, start) with the running maximum of their ends, so that a record finds the regions it overlaps: the first
// whose running maximum lies behind the record's first base, up to the first that starts behind its last.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "snp.h"

namespace ngm {
namespace cnt {

constexpr int kDefaultMinQual = 27;   // slamdunk count's -q

struct Region { int32_t contig; uint32_t start, end; std::string name; char strand; };

// ---- the BED file -----------------------------------------------------------------------------------------------------------------
// a decimal number of at most 10 digits that fits 32 bits
inline bool parse_u32(const std::string &s, uint32_t *out) {
	if (s.empty() || s.size() > 10) return false;
	uint64_t v = 0;
	for (char ch : s) { if (ch < '0' || ch > '9') return false; v = v * 10u + (uint64_t) (ch - '0'); }
	if (v > 0xffffffffull) return false;
	*out = (uint32_t) v;
	return true;
}

// the regions of a BED text over the contigs given, in the file's order; false with "line <n>: <reason>" in *err for the first line refused
inline bool parse_bed(const std::string &text, int n_ref, const char *const *ref_name, const uint32_t *ref_len, std::vector<Region> &out, std::string *err) {
	out.clear();
	size_t at = 0, line_no = 0;
	auto fail = [&](const std::string &why) { *err = "line " + std::to_string(line_no) + ": " + why; out.clear(); return false; };
	while (at < text.size()) {
		size_t nl = text.find('\n', at);
		if (nl == std::string::npos) nl = text.size();
		std::string line = text.substr(at, nl - at);
		at = nl + 1;
		++line_no;
		if (!line.empty() && line.back() == '\r') line.pop_back();
		if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
		std::vector<std::string> f;
		for (size_t b = 0;;) {
			const size_t t = line.find('\t', b);
			if (t == std::string::npos) { f.push_back(line.substr(b)); break; }
			f.push_back(line.substr(b, t - b));
			b = t + 1;
		}
		if (f.size() < 3) return fail("it has fewer than 3 tab-separated columns");
		Region r;
		r.contig = -1;
		for (int c = 0; c < n_ref; ++c) if (f[0] == ref_name[c]) { r.contig = c; break; }
		if (r.contig < 0) return fail("contig " + f[0] + " is not in the reference");
		if (!parse_u32(f[1], &r.start)) return fail("its start " + f[1] + " is not a number");
		if (!parse_u32(f[2], &r.end)) return fail("its end " + f[2] + " is not a number");
		if (r.start >= r.end) return fail("its start is not in front of its end");
		if (r.end > ref_len[r.contig]) return fail("its end lies behind the contig's last base (" + std::to_string(ref_len[r.contig]) + " bases)");
		r.name = f.size() > 3 ? f[3] : std::string(".");
		const std::string strand = f.size() > 5 ? f[5] : std::string(".");
		if (strand != "+" && strand != "-" && strand != ".") return fail("its strand " + strand + " is not +, - or .");
		r.strand = strand[0];
		out.push_back(r);
	}
	if (out.empty()) { line_no = 0; return fail("the file has no region"); }
	return true;
}

// ---- the tables -------------------------------------------------------------------------------------------------------------------
// pointers into host or device memory
struct Layout {
	const uint32_t *iv_start, *iv_end;   // the merged intervals, contig by contig, ascending
	const uint64_t *iv_slot;             // the slot of an interval's first base
	const uint32_t *contig_iv;           // [n_ref + 1] a contig's intervals
	const uint32_t *rs_start, *rs_end, *rs_maxend, *rs_index;   // the regions sorted by (contig, start): running maximum of end, index in the file
	const uint8_t *rs_take;              // bit 0: takes forward records, bit 1: reverse records
	const uint32_t *contig_rs;           // [n_ref + 1] a contig's regions
	const uint32_t *ref_len;             // [n_ref]
	const uint32_t *genome;              // 4-bit classes, 8 per dword (snp.h)
	const uint64_t *start;               // [n_ref] base offset of a contig in genome
	int n_ref, min_qual;
};

NGM_COV_HD inline uint8_t take_of(char strand) { return strand == '+' ? 1u : strand == '-' ? 2u : 3u; }

struct Tables {
	std::vector<uint32_t> iv_start, iv_end, contig_iv, rs_start, rs_end, rs_maxend, rs_index, contig_rs;
	std::vector<uint64_t> iv_slot;
	std::vector<uint8_t> rs_take;
	uint64_t slots = 0;

	void build(const std::vector<Region> &regions, int n_ref) {
		std::vector<uint32_t> order(regions.size());
		for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t) i;
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
			return regions[a].contig != regions[b].contig ? regions[a].contig < regions[b].contig : regions[a].start < regions[b].start;
		});
		contig_iv.assign((size_t) n_ref + 1, 0); contig_rs.assign((size_t) n_ref + 1, 0);
		iv_start.clear(); iv_end.clear(); iv_slot.clear(); rs_start.clear(); rs_end.clear(); rs_maxend.clear(); rs_index.clear(); rs_take.clear();
		slots = 0;
		size_t k = 0;
		for (int c = 0; c < n_ref; ++c) {
			contig_iv[c] = (uint32_t) iv_start.size(); contig_rs[c] = (uint32_t) rs_start.size();
			uint32_t maxend = 0;
			bool open = false;
			for (; k < order.size() && regions[order[k]].contig == c; ++k) {
				const Region &r = regions[order[k]];
				if (open && r.start <= iv_end.back()) iv_end.back() = std::max(iv_end.back(), r.end);
				else {
					if (open) slots += iv_end.back() - iv_start.back();
					iv_start.push_back(r.start); iv_end.push_back(r.end); iv_slot.push_back(slots);
					open = true;
				}
				maxend = std::max(maxend, r.end);
				rs_start.push_back(r.start); rs_end.push_back(r.end); rs_maxend.push_back(maxend); rs_index.push_back(order[k]); rs_take.push_back(take_of(r.strand));
			}
			if (open) slots += iv_end.back() - iv_start.back();
		}
		contig_iv[n_ref] = (uint32_t) iv_start.size(); contig_rs[n_ref] = (uint32_t) rs_start.size();
	}
	Layout layout(const uint32_t *ref_len, const uint32_t *genome, const uint64_t *start, int n_ref, int min_qual) const {
		return Layout{iv_start.data(), iv_end.data(), iv_slot.data(), contig_iv.data(), rs_start.data(), rs_end.data(), rs_maxend.data(), rs_index.data(), rs_take.data(),
				contig_rs.data(), ref_len, genome, start, n_ref, min_qual};
	}
};

// the slot of position p of contig c; false when no region covers it
NGM_COV_HD inline bool slot_of(const Layout &L, int c, uint32_t p, uint64_t *slot) {
	uint32_t lo = L.contig_iv[c], hi = L.contig_iv[c + 1];
	while (lo < hi) {   // the first interval that ends behind p
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (L.iv_end[mid] > p) hi = mid; else lo = mid + 1;
	}
	if (lo == L.contig_iv[c + 1] || L.iv_start[lo] > p) return false;
	*slot = L.iv_slot[lo] + (uint64_t) (p - L.iv_start[lo]);
	return true;
}

// ---- one record -------------------------------------------------------------------------------------------------------------------
// a record on the host
struct HostRec {
	int contig; int64_t pos0; const char *cigar; uint32_t cigar_len, seq_len;
	const char *seq, *qual;
	char base(uint32_t i) const { return seq[i]; }
	bool qual_ok(uint32_t i, int min_qual) const { return !qual || (int) (unsigned char) qual[i] - 33 >= min_qual; }
};

// the reference class under contig position p, the dword that holds it read once (w_at, w: the caller's cache, w_at = ~0 at first)
NGM_COV_HD inline uint32_t class_at(const Layout &L, uint64_t g, uint64_t &w_at, uint32_t &w) {
	if ((g >> 3) != w_at) { w_at = g >> 3; w = L.genome[w_at]; }
	return (w >> (4u * (uint32_t) (g & 7u))) & 15u;
}

// One record into the counters.  sink.slot(i): +1 on counter i of the per-base array (2 * slot: cov, 2 * slot + 1: conv); sink.region(i):
// +1 on counter i of the per-region array (2 * R: reads, 2 * R + 1: tc_reads).  stat[0]: 1 when a region took the record, stat[1]: its
// eligible columns inside the regions' union, stat[2]: the conversions among them.
template <typename RecT, typename Sink>
NGM_COV_HD inline void add_record(const Layout &L, const RecT &rec, bool reverse, Sink &sink, uint32_t stat[3]) {
	stat[0] = stat[1] = stat[2] = 0;
	const int c = rec.contig;
	if (c < 0 || c >= L.n_ref || rec.pos0 < 0) return;   // (never from the validated arrays; the mapper's records have a contig)
	const int64_t len = (int64_t) L.ref_len[c];
	int64_t lo = -1, hi = -1;   // the record's first and last aligned base (hi exclusive)
	snp::walk_segments(rec.pos0, rec.cigar, rec.cigar_len, len, [&](int64_t b, int64_t e, uint64_t) { if (lo < 0) lo = b; hi = e; });
	if (lo < 0) return;
	const uint32_t i1 = L.contig_iv[c + 1];
	uint32_t k = L.contig_iv[c];
	for (uint32_t h = i1; k < h;) {   // the first interval that ends behind lo
		const uint32_t mid = k + ((h - k) >> 1);
		if ((int64_t) L.iv_end[mid] > lo) h = mid; else k = mid + 1;
	}
	if (k == i1 || (int64_t) L.iv_start[k] >= hi) return;
	const uint32_t want = reverse ? 0u : 3u, to = reverse ? 2u : 1u;   // T read as C, or A read as G
	const uint64_t g0 = L.start[c];
	uint64_t w_at = ~0ull;
	uint32_t w = 0, eligible = 0, conv = 0;
	// is the column at p, read offset ri, eligible (1), a conversion (2) or neither (0)
	auto column = [&](int64_t p, uint64_t ri) -> int {
		if (class_at(L, g0 + (uint64_t) p, w_at, w) != want) return 0;
		const uint32_t b = snp::read_class_of(rec.base((uint32_t) ri));
		if (b > 3u || !rec.qual_ok((uint32_t) ri, L.min_qual)) return 0;
		return b == to ? 2 : 1;
	};
	snp::walk_segments(rec.pos0, rec.cigar, rec.cigar_len, len, [&](int64_t b, int64_t e, uint64_t ri0) {
		int64_t p = b;
		while (p < e && k < i1) {   // (segments ascend, and so does k)
			if ((int64_t) L.iv_end[k] <= p) { ++k; continue; }
			if ((int64_t) L.iv_start[k] >= e) break;
			const int64_t s = p > (int64_t) L.iv_start[k] ? p : (int64_t) L.iv_start[k], t = e < (int64_t) L.iv_end[k] ? e : (int64_t) L.iv_end[k];
			uint64_t slot = L.iv_slot[k] + (uint64_t) (s - (int64_t) L.iv_start[k]);
			for (int64_t q = s; q < t; ++q, ++slot) {
				const uint64_t ri = ri0 + (uint64_t) (q - b);
				if (ri >= (uint64_t) rec.seq_len) break;   // (a validated record never runs out of bases)
				const int what = column(q, ri);
				if (!what) continue;
				sink.slot(2u * slot); ++eligible;
				if (what == 2) { sink.slot(2u * slot + 1u); ++conv; }
			}
			p = t;
		}
	});
	stat[1] = eligible; stat[2] = conv;
	// the regions the record overlaps
	const uint32_t r1 = L.contig_rs[c + 1];
	uint32_t j = L.contig_rs[c];
	for (uint32_t h = r1; j < h;) {   // the first region whose running maximum of end lies behind lo
		const uint32_t mid = j + ((h - j) >> 1);
		if ((int64_t) L.rs_maxend[mid] > lo) h = mid; else j = mid + 1;
	}
	const uint8_t mine = reverse ? 2u : 1u;
	for (; j < r1 && (int64_t) L.rs_start[j] < hi; ++j) {
		if ((int64_t) L.rs_end[j] <= lo || !(L.rs_take[j] & mine)) continue;
		const int64_t rs = (int64_t) L.rs_start[j], re = (int64_t) L.rs_end[j];
		bool has_m = false, has_conv = false;
		snp::walk_segments(rec.pos0, rec.cigar, rec.cigar_len, len, [&](int64_t b, int64_t e, uint64_t ri0) {
			const int64_t s = b > rs ? b : rs, t = e < re ? e : re;
			if (s >= t) return;
			has_m = true;
			if (!conv || has_conv) return;   // (a conversion inside a region is one inside the union)
			for (int64_t q = s; q < t; ++q) {
				const uint64_t ri = ri0 + (uint64_t) (q - b);
				if (ri >= (uint64_t) rec.seq_len) break;
				if (column(q, ri) == 2) { has_conv = true; break; }
			}
		});
		if (!has_m) continue;
		stat[0] = 1;
		sink.region(2u * (uint64_t) L.rs_index[j]);
		if (has_conv) sink.region(2u * (uint64_t) L.rs_index[j] + 1u);
	}
}

// the sink of the host twin
struct HostSink {
	uint32_t *cnt; uint64_t *reg;
	void slot(uint64_t i) { cnt[i] += 1u; }
	void region(uint64_t i) { reg[i] += 1u; }
};

// ---- the finish -------------------------------------------------------------------------------------------------------------------
// does a region of this kind sum the base of reference class cls
NGM_COV_HD inline bool class_counts(uint8_t take, uint32_t cls) { return (cls == 3u && (take & 1u)) || (cls == 0u && (take & 2u)); }
NGM_COV_HD inline bool mask_bit(const uint32_t *mask, uint64_t slot) { return (mask[slot >> 5] >> (uint32_t) (slot & 31u)) & 1u; }

// host: the four sums of one region -- t_bases, masked, cov_on_ts, conv_on_ts -- into out[0..3]
inline void reduce_host(const Layout &L, const Region &r, const uint32_t *cnt, const uint32_t *mask, int64_t out[4]) {
	out[0] = out[1] = out[2] = out[3] = 0;
	uint64_t slot = 0;
	if (!slot_of(L, r.contig, r.start, &slot)) return;   // (never: a region lies inside one interval)
	const uint8_t take = take_of(r.strand);
	for (uint32_t p = r.start; p < r.end; ++p, ++slot) {
		if (!class_counts(take, snp::packed_class(L.genome, L.start[r.contig] + p))) continue;
		if (mask_bit(mask, slot)) { out[1] += 1; continue; }
		out[0] += 1; out[2] += cnt[2u * slot]; out[3] += cnt[2u * slot + 1u];
	}
}

inline const char *header() { return "#chrom\tstart\tend\tname\tstrand\tt_bases\tmasked\tcov_on_ts\tconv_on_ts\treads\ttc_reads\n"; }

// the file: six numbers per region (t_bases, masked, cov_on_ts, conv_on_ts, reads, tc_reads), regions in the file's order
inline std::string serialise(const std::vector<Region> &regions, const char *const *ref_name, const int64_t *six) {
	std::string s = header();
	for (size_t i = 0; i < regions.size(); ++i) {
		const Region &r = regions[i];
		s += ref_name[r.contig]; s.push_back('\t'); cov::put_u64(s, r.start); s.push_back('\t'); cov::put_u64(s, r.end); s.push_back('\t'); s += r.name; s.push_back('\t'); s.push_back(r.strand);
		for (int k = 0; k < 6; ++k) { s.push_back('\t'); cov::put_u64(s, (unsigned long long) six[6 * i + (size_t) k]); }
		s.push_back('\n');
	}
	return s;
}

}  // namespace cnt
}  // namespace ngm
