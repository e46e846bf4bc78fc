// CPU-only driver for tests/test_host_units.py: the header-only host pieces of the product that need no GPU.
//   bam <out.bam>        a small BAM file written with csrc/bam_writer.h (header, dictionary, records in several BGZF chunks, EOF)
//   pool                 ngm::ThreadPool::parallel_for: sums, concurrent callers, nested use
//   format <spec> [out.bam]   the host formatter of `ngm-hip` (csrc/cli_format.h) over the records a text file describes:
//                        opt <key> <value> (q: bytes per read row, before the records) | contig <name> <bases> |
//                        rec <name> <row or -> <qualities or *> <seq_len> <unit> <polya> [<qual_len>: the length of the quality string as the parser
//                        holds it, where the row holds less of it], followed by topn lines: hit <mapped> <contig> <pos> <reverse> <mapq> <score>
//                        <identity> <nm> <qstart> <qend> <n_candidates> <n_best> <max_votes> <pair_flags> <cigar or -> <md or ->.  Prints the SAM text (with out.bam: writes the records as a BAM file instead), what the
//                        --coverage / --snp callbacks got ("#cov", "#snp"), and "#counts total mapped written pairs broken insert_sum"
#include <atomic>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../nextgenmap_amd/csrc/bam_writer.h"
#include "../../nextgenmap_amd/csrc/cli_format.h"
#include "../../nextgenmap_amd/csrc/thread_pool.h"

static int write_bam(const char *path) {
	std::string raw, file;
	ngm::bam::put_header(raw, "@HD\tVN:1.0\tSO:unsorted\n@PG\tID:ngm\n", {"chr1", "chrTwo"}, {1000000, 54321});
	if (!ngm::bam::bgzf_compress(raw.data(), raw.size(), file)) return 2;
	// three chunks of records, each compressed on its own (as the formatter threads do): they must concatenate into one file
	for (int chunk = 0; chunk < 3; ++chunk) {
		std::string recs;
		for (int i = 0; i < 700; ++i) {
			const int id = chunk * 700 + i;
			char name[32];
			const int nl = snprintf(name, sizeof(name), "read%05d", id);
			std::string seq(100 + id % 51, 'A');
			for (size_t t = 0; t < seq.size(); ++t) seq[t] = "ACGTN"[(id + 3 * t) % 5];
			std::string qual(seq.size(), 'I');
			for (size_t t = 0; t < qual.size(); ++t) qual[t] = (char) (33 + (id + t) % 40);
			char cigar[64];
			snprintf(cigar, sizeof(cigar), "%dS%dM2I%dM1D%dM", id % 7 + 1, 20, 30, (int) seq.size() - 53 - (id % 7 + 1));
			ngm::bam::Tags tg;
			tg.add_int("AS", 1234 - id); tg.add_int("NM", id % 9); tg.add_float("XI", 0.9876f); tg.add_string("MD", "50A49", 5);
			const bool unmapped = id % 97 == 0;
			ngm::bam::put_record(recs, name, (size_t) nl, unmapped ? 4u : (id % 2 ? 16u : 0u), unmapped ? -1 : id % 2, unmapped ? -1 : 1000 + 37 * id, unmapped ? 0 : 60,
					unmapped ? nullptr : cigar, seq.data(), seq.size(), id % 5 == 0 ? nullptr : qual.data(), -1, -1, 0, tg);
		}
		if (!ngm::bam::bgzf_compress(recs.data(), recs.size(), file)) return 3;
	}
	ngm::bam::bgzf_eof(file);
	FILE *f = fopen(path, "wb");
	if (!f) return 4;
	fwrite(file.data(), 1, file.size(), f);
	fclose(f);
	printf("min_bin %u %u %u %u %u\n", ngm::bam::min_bin(0, 1), ngm::bam::min_bin(16383, 16385), ngm::bam::min_bin(1 << 20, (1 << 20) + 150), ngm::bam::min_bin(-1, -1),
			ngm::bam::min_bin(100000000, 100000200));
	return 0;
}

static int test_pool() {
	ngm::ThreadPool &pool = ngm::ThreadPool::instance();
	// every index exactly once, any grain
	for (int n : {0, 1, 7, 1000, 100003}) for (int grain : {1, 64, 4096}) {
		std::vector<std::atomic<int>> seen(n);
		for (auto &s : seen) s = 0;
		pool.parallel_for(n, [&](int lo, int hi) { for (int i = lo; i < hi; ++i) seen[i].fetch_add(1); }, grain);
		for (int i = 0; i < n; ++i) if (seen[i] != 1) { printf("pool: index %d of %d seen %d times (grain %d)\n", i, n, (int) seen[i], grain); return 1; }
	}
	// several callers at once (the mapper instances and the CLI stages share the pool), one of them nesting
	std::atomic<long long> total{0};
	std::vector<std::thread> callers;
	for (int c = 0; c < 6; ++c) callers.emplace_back([&, c] {
		for (int rep = 0; rep < 20; ++rep) {
			long long local = 0;
			std::atomic<long long> sum{0};
			pool.parallel_for(50000, [&](int lo, int hi) {
				long long s = 0;
				for (int i = lo; i < hi; ++i) s += i;
				if (c == 0 && lo == 0) pool.parallel_for(1000, [&](int a, int b) { sum += (b - a); }, 100);  // nested
				sum += s;
			}, 512);
			local = sum;
			total += local - (c == 0 ? 1000 : 0);
		}
	});
	for (auto &t : callers) t.join();
	const long long expect = 6LL * 20 * (50000LL * 49999 / 2);
	printf("pool threads %d total %lld expect %lld\n", pool.size(), (long long) total, expect);
	return total == expect ? 0 : 1;
}

static int format_records(const char *spec, const char *bam_out) {
	using ngm::cli::HostFormatter;
	HostFormatter f;
	f.q = 16;
	std::vector<std::string> contig_seq;
	struct Text { std::string name, row, qual; long qual_len; };
	std::vector<Text> text;
	std::vector<ngm::cli::Rec> recs;
	std::vector<ngm_hit> hits;
	std::vector<std::string> cig, md;
	bool cov = false, snp = false;
	std::ifstream in(spec);
	for (std::string line; std::getline(in, line);) {
		std::istringstream ls(line);
		std::string kind;
		if (!(ls >> kind) || kind[0] == '#') continue;
		if (kind == "opt") {
			std::string k, v;
			ls >> k >> v;
			if (k == "min_identity") f.min_identity = std::stof(v); else if (k == "min_residues") f.min_residues = std::stof(v); else if (k == "min_mq") f.min_mq = std::stoi(v);
			else if (k == "paired") f.paired = std::stoi(v); else if (k == "topn") f.topn = std::stoi(v); else if (k == "strata") f.strata = std::stoi(v);
			else if (k == "clip") f.clip = std::stoi(v); else if (k == "no_unal") f.no_unal = std::stoi(v); else if (k == "bs_mapping") f.bs_mapping = std::stoi(v);
			else if (k == "slam_seq") f.slam_seq = std::stoi(v); else if (k == "variant") f.variant = std::stoi(v); else if (k == "xa_tag") f.xa_tag = std::stoi(v) != 0;
			else if (k == "rg") f.set_read_group(v); else if (k == "min_insert") f.min_insert = std::stoi(v); else if (k == "max_insert") f.max_insert = std::stoi(v);
			else if (k == "q") { f.q = std::stoi(v); if (f.q < 1 || !text.empty()) { fprintf(stderr, "bad q\n"); return 65; } }
			else if (k == "coverage") cov = std::stoi(v) != 0; else if (k == "snp") snp = std::stoi(v) != 0;
			else { fprintf(stderr, "unknown option %s\n", k.c_str()); return 65; }
		} else if (kind == "contig") {
			std::string name, bases;
			ls >> name >> bases;
			f.contig_names.push_back(name); contig_seq.push_back(bases);
		} else if (kind == "rec") {
			Text t;
			unsigned seq_len = 0, unit = 0, polya = 0;
			ls >> t.name >> t.row >> t.qual >> seq_len >> unit >> polya;
			if (!ls) { fprintf(stderr, "bad rec line: %s\n", line.c_str()); return 65; }
			if (t.row == "-") t.row.clear();
			if (t.qual == "*") t.qual.clear();
			if (!(ls >> t.qual_len)) t.qual_len = (long) t.qual.size();
			if (t.qual_len < 0 || t.qual_len > 0x7FFF || (size_t) std::min<long>(t.qual_len, f.q - 1) > t.qual.size()) { fprintf(stderr, "bad quality length: %s\n", line.c_str()); return 65; }
			t.row.resize((size_t) f.q, '\0');
			text.push_back(t);
			recs.push_back(ngm::cli::Rec{nullptr, nullptr, nullptr, 0, seq_len, 0, (uint8_t) unit, (uint16_t) polya});
		} else if (kind == "hit") {
			ngm_hit h{};
			std::string c, m;
			ls >> h.mapped >> h.contig >> h.pos >> h.reverse >> h.mapq >> h.score >> h.identity >> h.nm >> h.qstart >> h.qend >> h.n_candidates >> h.n_best >> h.max_votes >> h.pair_flags >> c >> m;
			if (!ls) { fprintf(stderr, "bad hit line: %s\n", line.c_str()); return 65; }
			if (c == "-") c.clear();
			if (m == "-") m.clear();
			hits.push_back(h); cig.push_back(c); md.push_back(m);
		} else { fprintf(stderr, "unknown line: %s\n", line.c_str()); return 65; }
	}
	f.bam = bam_out != nullptr;
	f.stride = (size_t) 4 * f.q;
	const size_t n = recs.size();
	if (hits.size() != n * (size_t) f.topn) { fprintf(stderr, "%zu records need %zu hits, not %zu\n", n, n * (size_t) f.topn, hits.size()); return 65; }
	std::vector<char> rows(n * (size_t) f.q + 1, '\0'), cigs(hits.size() * f.stride + 1, '\0'), mds(hits.size() * f.stride + 1, '\0');
	for (size_t i = 0; i < n; ++i) {
		memcpy(&rows[i * (size_t) f.q], text[i].row.data(), (size_t) f.q);
		recs[i].name = text[i].name.data(); recs[i].name_len = (uint32_t) text[i].name.size();
		recs[i].qual = text[i].qual.data(); recs[i].qual_len = (uint32_t) text[i].qual_len;
	}
	for (size_t e = 0; e < hits.size(); ++e) {
		if (cig[e].size() >= f.stride || md[e].size() >= f.stride) return 65;
		memcpy(&cigs[e * f.stride], cig[e].data(), cig[e].size()); memcpy(&mds[e * f.stride], md[e].data(), md[e].size());
	}
	f.ref_classes = [&](int contig, uint64_t pos, int span, uint8_t *out) {
		for (int k = 0; k < span; ++k) {
			const char ch = pos + (uint64_t) k < contig_seq[contig].size() ? contig_seq[contig][pos + (uint64_t) k] : 'N';
			out[k] = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : ch == 'N' ? 5 : 4;
		}
	};
	std::string side;
	if (cov) f.add_coverage = [&](const ngm::cli::CovAcc &a) {
		side += "#cov";
		for (size_t i = 0; i < a.ref.size(); ++i) side += " " + std::to_string(a.ref[i]) + ":" + std::to_string(a.pos[i]) + ":" + a.text.substr(a.off[i], a.off[i + 1] - a.off[i]);
		side += "\n";
	};
	if (snp) f.add_snp = [&](const ngm::cli::SnpAcc &a, bool has_qual) {
		side += has_qual ? "#snp qual" : "#snp noqual";
		if (a.qual.size() != (has_qual ? a.seq.size() : 0)) side += " QUALITY-LENGTH-DIFFERS";
		for (size_t i = 0; i < a.ref.size(); ++i) {
			side += " " + std::to_string(a.ref[i]) + ":" + std::to_string(a.pos[i]) + ":" + a.text.substr(a.off[i], a.off[i + 1] - a.off[i]) + ":" + a.seq.substr(a.seq_off[i], a.seq_off[i + 1] - a.seq_off[i]);
			if (has_qual) side += ":" + a.qual.substr(a.seq_off[i], a.seq_off[i + 1] - a.seq_off[i]);
		}
		side += "\n";
	};
	std::string out;
	HostFormatter::Counts c;
	f.format_range(HostFormatter::Input{recs.data(), hits.data(), rows.data(), cigs.data(), mds.data()}, 0, (int) n, out, c);
	if (bam_out) {
		std::string raw, file;
		std::vector<uint64_t> lens;
		for (const std::string &b : contig_seq) lens.push_back(b.size());
		ngm::bam::put_header(raw, "@HD\tVN:1.0\tSO:unsorted\n", f.contig_names, lens);
		raw += out;
		if (!ngm::bam::bgzf_compress(raw.data(), raw.size(), file)) return 2;
		ngm::bam::bgzf_eof(file);
		std::ofstream(bam_out, std::ios::binary).write(file.data(), (std::streamsize) file.size());
	} else fwrite(out.data(), 1, out.size(), stdout);
	fwrite(side.data(), 1, side.size(), stdout);
	printf("#counts %zu %zu %zu %llu %llu %llu\n", c.total, c.mapped, c.written, (unsigned long long) c.pair[0], (unsigned long long) c.pair[1], (unsigned long long) c.pair[2]);
	return 0;
}

int main(int argc, char **argv) {
	if (argc >= 3 && !strcmp(argv[1], "format")) return format_records(argv[2], argc >= 4 ? argv[3] : nullptr);
	if (argc >= 3 && !strcmp(argv[1], "bam")) return write_bam(argv[2]);
	if (argc >= 2 && !strcmp(argv[1], "pool")) return test_pool();
	return 64;
}
