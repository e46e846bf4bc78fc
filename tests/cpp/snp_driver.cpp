// snp_driver.cpp -- the host-only parts of `ngm-hip --snp` (nextgenmap_amd/csrc/snp.h) as a stand-alone program, for
// tests/test_snp_host.py: plain g++, no GPU.
//   snp_driver file <in> <out>    in: "<n_ref>", n_ref lines "<name> <sequence>", a line "<min_cov> <min_frac> <min_qual>", then one record
//                                 per line "<ref_id> <pos0> <CIGAR> <sequence> <qualities>" ("-": an empty CIGAR or sequence, "*": no
//                                 qualities).  Every record passes the checks, is walked into counter arrays on the host, and the arrays
//                                 are serialised behind the header into <out>; prints "<alignments> <mismatching bases> <calls> <covered>".
//   snp_driver check <in>         the same input; prints one line per record: "<code> <message>" of the checks.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/snp.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;

int main(int argc, char **argv) {
	if (argc < 3) { fprintf(stderr, "usage: snp_driver file <in> <out> | check <in>\n"); return 2; }
	const std::string mode = argv[1];
	std::ifstream in(argv[2]);
	if (!in) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
	int n_ref = 0;
	in >> n_ref;
	std::vector<std::string> names((size_t) n_ref), seqs((size_t) n_ref);
	std::vector<uint32_t> lens((size_t) n_ref);
	for (int c = 0; c < n_ref; ++c) { in >> names[c] >> seqs[c]; if (seqs[c] == "-") seqs[c].clear(); lens[c] = (uint32_t) seqs[c].size(); }
	std::vector<const char *> name_ptr, seq_ptr;
	for (const std::string &s : names) name_ptr.push_back(s.c_str());
	for (const std::string &s : seqs) seq_ptr.push_back(s.c_str());
	long long min_cov = 0, min_qual = 0;
	std::string frac_text;
	in >> min_cov >> frac_text >> min_qual;
	const sn::Rule rule{(uint32_t) min_cov, strtod(frac_text.c_str(), nullptr), (int) min_qual};
	const std::vector<uint64_t> off = cv::contig_offsets(lens.data(), n_ref);
	std::vector<uint64_t> start;
	const std::vector<uint32_t> genome = sn::pack_reference(seq_ptr.data(), lens.data(), n_ref, start);
	std::vector<int32_t> diff((size_t) off[n_ref], 0);
	std::vector<uint32_t> alt((size_t) off[n_ref] * 3, 0u);
	long long ref_id, pos0;
	std::string cigar, seq, qual;
	size_t i = 0;
	uint64_t counted = 0;
	while (in >> ref_id >> pos0 >> cigar >> seq >> qual) {
		if (cigar == "-") cigar.clear();
		if (seq == "-") seq.clear();
		const bool has_qual = qual != "*";
		if (qual == "-") qual.clear();
		int code = sn::check_alignment((int32_t) ref_id, (int32_t) pos0, cigar.data(), (uint32_t) cigar.size(), n_ref, seq.size());
		if (code == cv::kOk && has_qual && qual.size() != seq.size()) code = sn::kQualLength;
		if (mode == "check") { printf("%d %s\n", code, sn::why(code)); ++i; continue; }
		if (code != cv::kOk) { fprintf(stderr, "record %zu: %s\n", i, sn::why(code)); return 1; }
		counted += sn::add_host(diff.data(), alt.data(), off.data(), lens.data(), genome.data(), start.data(), rule.min_qual, (int32_t) ref_id, (int32_t) pos0, cigar.data(),
				(uint32_t) cigar.size(), seq.data(), has_qual ? qual.data() : nullptr);
		++i;
	}
	if (mode == "check") return 0;
	if (mode != "file" || argc < 4) { fprintf(stderr, "unknown mode\n"); return 2; }
	std::string text = sn::header(n_ref, name_ptr.data(), lens.data(), rule, frac_text.c_str());
	uint64_t calls = 0, covered = 0;
	sn::serialise(diff.data(), alt.data(), off.data(), n_ref, name_ptr.data(), genome.data(), start.data(), rule, text, &calls, &covered);
	std::ofstream out(argv[3], std::ios::binary);
	out.write(text.data(), (std::streamsize) text.size());
	if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
	printf("%zu %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", i, counted, calls, covered);
	return 0;
}
