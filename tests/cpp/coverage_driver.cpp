// coverage_driver.cpp -- the host-only parts of `ngm-hip --coverage` (nextgenmap_amd/csrc/coverage.h) as a stand-alone program, for
// tests/test_coverage_host.py: plain g++, no GPU.
//   coverage_driver file <in> <out>    in: "<n_ref>", n_ref lines "<name> <length>", then one alignment per line "<ref_id> <pos0> <CIGAR>"
//                                      ("-": an empty CIGAR).  Every alignment passes the validator, is walked into a counter array on the
//                                      host, and the array is serialised into <out>; prints "<covered bases> <runs>".
//   coverage_driver check <in>         the same input; prints one line per alignment: "<code> <message>" of the validator.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/coverage.h"

namespace cv = ngm::cov;

int main(int argc, char **argv) {
	if (argc < 3) { fprintf(stderr, "usage: coverage_driver file <in> <out> | check <in>\n"); return 2; }
	const std::string mode = argv[1];
	std::ifstream in(argv[2]);
	if (!in) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
	int n_ref = 0;
	in >> n_ref;
	std::vector<std::string> names((size_t) n_ref);
	std::vector<uint32_t> lens((size_t) n_ref);
	for (int c = 0; c < n_ref; ++c) in >> names[c] >> lens[c];
	std::vector<const char *> name_ptr;
	for (const std::string &s : names) name_ptr.push_back(s.c_str());
	const std::vector<uint64_t> off = cv::contig_offsets(lens.data(), n_ref);
	std::vector<int32_t> counters((size_t) off[n_ref], 0);
	long long ref_id, pos0;
	std::string cigar;
	size_t i = 0;
	while (in >> ref_id >> pos0 >> cigar) {
		if (cigar == "-") cigar.clear();
		const int code = cv::check_alignment((int32_t) ref_id, (int32_t) pos0, cigar.data(), (uint32_t) cigar.size(), n_ref);
		if (mode == "check") { printf("%d %s\n", code, cv::why(code)); ++i; continue; }
		if (code != cv::kOk) { fprintf(stderr, "alignment %zu: %s\n", i, cv::why(code)); return 1; }
		cv::add_host(counters.data(), off.data(), lens.data(), (int32_t) ref_id, (int32_t) pos0, cigar.data(), (uint32_t) cigar.size());
		++i;
	}
	if (mode == "check") return 0;
	if (mode != "file" || argc < 4) { fprintf(stderr, "unknown mode\n"); return 2; }
	std::string text;
	uint64_t covered = 0, runs = 0;
	cv::serialise(counters.data(), off.data(), n_ref, name_ptr.data(), text, &covered, &runs);
	for (int c = 0; c < n_ref; ++c) if (cv::contig_of(off.data(), n_ref, off[c]) != c || cv::contig_of(off.data(), n_ref, off[c + 1] - 1) != c) { fprintf(stderr, "contig_of is wrong for contig %d\n", c); return 1; }
	std::ofstream out(argv[3], std::ios::binary);
	out.write(text.data(), (std::streamsize) text.size());
	if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
	printf("%" PRIu64 " %" PRIu64 "\n", covered, runs);
	return 0;
}
