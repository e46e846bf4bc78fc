// methyl_driver.cpp -- the host-only parts of `ngm-hip --bs-mapping --methyl` (nextgenmap_amd/csrc/methyl.h) as a stand-alone program, for
// tests/test_methyl_host.py: plain g++, no GPU.  Everything is read from standard input.
//   methyl_driver file    "<n_ref>", n_ref lines "<name> <sequence>", a line "<min_qual> <min_depth> <context>", then one record per line
//                         "<ref_id> <pos0> <CIGAR> <sequence> <qualities> <bottom>" ("-": an empty CIGAR or sequence, "*": no qualities).
//                         Every record passes ngm_methyl_add's checks and is walked into a counter array on the host; the file is printed,
//                         then a line "stats <alignments> <lines> <CG meth> <CG unmeth> <CHG meth> <CHG unmeth> <CHH meth> <CHH unmeth>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/methyl.h"

namespace cv = ngm::cov;
namespace sn = ngm::snp;
namespace mt = ngm::met;

int main(int argc, char **argv) {
	if (argc < 2 || std::string(argv[1]) != "file") { fprintf(stderr, "usage: methyl_driver file\n"); return 2; }
	std::istream &in = std::cin;
	int n_ref = 0;
	in >> n_ref;
	std::vector<std::string> names((size_t) n_ref), seqs((size_t) n_ref);
	std::vector<uint32_t> lens((size_t) n_ref);
	for (int c = 0; c < n_ref; ++c) { in >> names[c] >> seqs[c]; if (seqs[c] == "-") seqs[c].clear(); lens[c] = (uint32_t) seqs[c].size(); }
	std::vector<const char *> name_ptr, seq_ptr;
	for (const std::string &s : names) name_ptr.push_back(s.c_str());
	for (const std::string &s : seqs) seq_ptr.push_back(s.c_str());
	long long min_qual = 0, min_depth = 0;
	std::string context;
	in >> min_qual >> min_depth >> context;
	const uint32_t selection = mt::selection_of(context.c_str());
	if (!selection || min_qual < 0 || min_qual > 93 || min_depth < 0) { fprintf(stderr, "bad parameters\n"); return 1; }
	std::vector<uint64_t> start;
	const std::vector<uint32_t> genome = sn::pack_reference(seq_ptr.data(), lens.data(), n_ref, start);
	const std::vector<uint64_t> off = mt::pair_offsets(lens.data(), n_ref);
	const mt::Layout L{off.data(), genome.data(), start.data(), n_ref, (int) min_qual};
	std::vector<uint32_t> cnt((size_t) off[(size_t) n_ref] * 2 + 1, 0u);
	uint64_t alignments = 0;
	long long ref_id, pos0;
	int bottom = 0;
	std::string cigar, seq, qual;
	mt::HostSink sink{cnt.data()};
	while (in >> ref_id >> pos0 >> cigar >> seq >> qual >> bottom) {
		if (cigar == "-") cigar.clear();
		if (seq == "-") seq.clear();
		const bool has_qual = qual != "*";
		if (qual == "-") qual.clear();
		int code = sn::check_alignment((int32_t) ref_id, (int32_t) pos0, cigar.data(), (uint32_t) cigar.size(), n_ref, seq.size());
		if (code == cv::kOk && has_qual && qual.size() != seq.size()) code = sn::kQualLength;
		if (code != cv::kOk) { fprintf(stderr, "record %" PRIu64 ": %s\n", alignments, sn::why(code)); return 1; }
		const mt::HostRec rec{(int) ref_id, (int64_t) pos0, cigar.data(), (uint32_t) cigar.size(), (uint32_t) seq.size(), seq.data(), has_qual ? qual.data() : nullptr};
		uint32_t st[2];
		mt::add_record(L, rec, bottom != 0, sink, st);
		++alignments;
	}
	std::string text;
	uint64_t lines = 0, sums[6] = {0, 0, 0, 0, 0, 0};
	mt::serialise(cnt.data(), off.data(), n_ref, name_ptr.data(), genome.data(), start.data(), (uint32_t) min_depth, selection, text, &lines, sums);
	fwrite(text.data(), 1, text.size(), stdout);
	printf("stats %" PRIu64 " %" PRIu64, alignments, lines);
	for (int k = 0; k < 6; ++k) printf(" %" PRIu64, sums[k]);
	printf("\n");
	return 0;
}
