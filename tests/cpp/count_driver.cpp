// count_driver.cpp -- the host-only parts of `ngm-hip --count` (nextgenmap_amd/csrc/count.h) as a stand-alone program, for
// tests/test_count_host.py: plain g++, no GPU.  Everything is read from standard input.
//   count_driver file     "<n_ref>", n_ref lines "<name> <sequence>", a line "<min_qual>", "<n_regions>", n_regions lines
//                         "<contig index> <start> <end> <name> <strand>", "<n_mask>", n_mask lines "<contig index> <position>", then one
//                         record per line "<ref_id> <pos0> <CIGAR> <sequence> <qualities> <reverse>" ("-": an empty CIGAR or sequence, "*": no
//                         qualities).  Every record passes ngm_count_add's checks and is walked into counter arrays on the host; the regions
//                         are summed and the file is printed, then a line "stats <alignments> <met a region> <eligible> <conversions> <masked>".
//   count_driver bed      "<n_ref>", n_ref lines "<name> <length>", then the BED text up to the end of the input; prints "ok <n>" and one
//                         line "<contig index> <start> <end> <name> <strand>" per region, or "error <message>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/count.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace ct = ngm::cnt;

int main(int argc, char **argv) {
	if (argc < 2) { fprintf(stderr, "usage: count_driver file | bed\n"); return 2; }
	const std::string mode = argv[1];
	std::istream &in = std::cin;
	int n_ref = 0;
	in >> n_ref;
	std::vector<std::string> names((size_t) n_ref), seqs((size_t) n_ref);
	std::vector<uint32_t> lens((size_t) n_ref);
	if (mode == "bed") {
		for (int c = 0; c < n_ref; ++c) in >> names[c] >> lens[c];
		in.get();   // (the end of the last length's line)
		const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		std::vector<const char *> name_ptr;
		for (const std::string &s : names) name_ptr.push_back(s.c_str());
		std::vector<ct::Region> regions;
		std::string err;
		if (!ct::parse_bed(text, n_ref, name_ptr.data(), lens.data(), regions, &err)) { printf("error %s\n", err.c_str()); return 0; }
		printf("ok %zu\n", regions.size());
		for (const ct::Region &r : regions) printf("%d %u %u %s %c\n", r.contig, r.start, r.end, r.name.c_str(), r.strand);
		return 0;
	}
	if (mode != "file") { fprintf(stderr, "unknown mode\n"); return 2; }
	for (int c = 0; c < n_ref; ++c) { in >> names[c] >> seqs[c]; if (seqs[c] == "-") seqs[c].clear(); lens[c] = (uint32_t) seqs[c].size(); }
	std::vector<const char *> name_ptr, seq_ptr;
	for (const std::string &s : names) name_ptr.push_back(s.c_str());
	for (const std::string &s : seqs) seq_ptr.push_back(s.c_str());
	long long min_qual = 0;
	size_t n_regions = 0, n_mask = 0;
	in >> min_qual >> n_regions;
	std::vector<ct::Region> regions(n_regions);
	for (ct::Region &r : regions) {
		std::string strand;
		in >> r.contig >> r.start >> r.end >> r.name >> strand;
		r.strand = strand[0];
	}
	std::vector<uint64_t> start;
	const std::vector<uint32_t> genome = sn::pack_reference(seq_ptr.data(), lens.data(), n_ref, start);
	ct::Tables tables;
	tables.build(regions, n_ref);
	const ct::Layout L = tables.layout(lens.data(), genome.data(), start.data(), n_ref, (int) min_qual);
	std::vector<uint32_t> cnt((size_t) tables.slots * 2 + 1, 0u), mask((size_t) (tables.slots + 31) / 32 + 1, 0u);
	std::vector<uint64_t> reg(n_regions * 2 + 1, 0u);
	uint64_t stats[5] = {0, 0, 0, 0, 0};
	in >> n_mask;
	for (size_t i = 0; i < n_mask; ++i) {
		long long c = 0, p = 0;
		in >> c >> p;
		uint64_t slot = 0;
		if (c < 0 || c >= n_ref || p < 0 || p >= (long long) lens[(size_t) c] || !ct::slot_of(L, (int) c, (uint32_t) p, &slot)) continue;
		if (!ct::mask_bit(mask.data(), slot)) { mask[(size_t) (slot >> 5)] |= 1u << (uint32_t) (slot & 31u); ++stats[4]; }
	}
	long long ref_id, pos0;
	int reverse = 0;
	std::string cigar, seq, qual;
	ct::HostSink sink{cnt.data(), reg.data()};
	while (in >> ref_id >> pos0 >> cigar >> seq >> qual >> reverse) {
		if (cigar == "-") cigar.clear();
		if (seq == "-") seq.clear();
		const bool has_qual = qual != "*";
		if (qual == "-") qual.clear();
		int code = sn::check_alignment((int32_t) ref_id, (int32_t) pos0, cigar.data(), (uint32_t) cigar.size(), n_ref, seq.size());
		if (code == cv::kOk && has_qual && qual.size() != seq.size()) code = sn::kQualLength;
		if (code != cv::kOk) { fprintf(stderr, "record %" PRIu64 ": %s\n", stats[0], sn::why(code)); return 1; }
		const ct::HostRec rec{(int) ref_id, (int64_t) pos0, cigar.data(), (uint32_t) cigar.size(), (uint32_t) seq.size(), seq.data(), has_qual ? qual.data() : nullptr};
		uint32_t st[3];
		ct::add_record(L, rec, reverse != 0, sink, st);
		++stats[0];
		for (int k = 0; k < 3; ++k) stats[1 + k] += st[k];
	}
	std::vector<int64_t> six(n_regions * 6 + 1, 0);
	for (size_t i = 0; i < n_regions; ++i) {
		ct::reduce_host(L, regions[i], cnt.data(), mask.data(), &six[6 * i]);
		six[6 * i + 4] = (int64_t) reg[2 * i]; six[6 * i + 5] = (int64_t) reg[2 * i + 1];
	}
	const std::string text = ct::serialise(regions, name_ptr.data(), six.data());
	fwrite(text.data(), 1, text.size(), stdout);
	printf("stats %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", stats[0], stats[1], stats[2], stats[3], stats[4]);
	return 0;
}
