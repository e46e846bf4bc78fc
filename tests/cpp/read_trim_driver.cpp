// read_trim_driver.cpp -- csrc/read_trim.h on a plain 4-line FASTQ file, without the GPU (tests/test_read_trim_host.py).
//   read_trim_driver <reads.fq> <trim5> <max_polya> <qry_max_len>
// One line per record: name, sequence, quality, polyA, discarded (tab-separated) -- the read as the mapper and the writers see it:
// the row's bases, the first `length` characters of the quality string behind the -5 prefix ('*': none), the bases --max-polya cut,
// 1 for a read without a sequence (the writers drop it).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/read_trim.h"

int main(int argc, char **argv) {
	if (argc != 5) { fprintf(stderr, "usage: read_trim_driver <reads.fq> <trim5> <max_polya> <qry_max_len>\n"); return 2; }
	ngm::trim::Options t;
	t.trim5 = atoi(argv[2]);
	t.max_polya = atoi(argv[3]);
	const int q = atoi(argv[4]);
	if (q < 2) { fprintf(stderr, "qry_max_len must be 2 or more\n"); return 2; }
	std::ifstream in(argv[1]);
	if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
	std::string head, seq_line, plus, qual_line;
	std::vector<char> row((size_t) q);
	while (std::getline(in, head) && std::getline(in, seq_line) && std::getline(in, plus) && std::getline(in, qual_line)) {
		if (head.empty() || head[0] != '@' || plus.empty() || plus[0] != '+') { fprintf(stderr, "not a 4-line FASTQ record: %s\n", head.c_str()); return 1; }
		size_t e = 1;
		while (e < head.size() && head[e] != ' ' && head[e] != '\t') ++e;
		const char *seq = seq_line.data(), *qual = qual_line.data();
		uint32_t seq_len = (uint32_t) seq_line.size(), qual_len = (uint32_t) qual_line.size();
		const int polya = ngm::trim::parse_read(t, q, seq, seq_len, qual, qual_len, row.data());
		const std::string bases(row.data(), strnlen(row.data(), (size_t) q));
		const std::string quals = qual_len == 0 ? std::string("*") : std::string(qual, std::min<size_t>(qual_len, bases.size()));
		printf("%s\t%s\t%s\t%d\t%d\n", head.substr(1, e - 1).c_str(), bases.c_str(), quals.c_str(), polya, seq_len == 0 ? 1 : 0);
	}
	return 0;
}
