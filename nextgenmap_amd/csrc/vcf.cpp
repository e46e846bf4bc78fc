// vcf.cpp -- the VCF reader of --vcf: VcfParser (src/parser/VcfParser.cpp) restated, with the lines split across the pool threads.
// The variants keep the file's order (the index build applies them in that order, PrefixTable.cpp:500-574).
// One deliberate difference: a VCF that cannot be opened is an error here; the reference logs it and builds without variants.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include <zlib.h>

#include "refindex.h"
#include "thread_pool.h"

namespace {
bool is_sequence(const char *s, size_t n) {  // VcfParser::isSequence: upper-case ACGTN only
	for (size_t i = 0; i < n; ++i)
		if (s[i] != 'A' && s[i] != 'C' && s[i] != 'G' && s[i] != 'T' && s[i] != 'N') return false;
	return true;
}

struct Chunk {
	std::vector<NgmVariant> v;  // ref_off / alt_off index `seq` of this chunk until the chunks are joined
	std::string seq, log;
};

// VcfParser::parse_line + add_line for one line (without its '\n'), line_num counted from 1
void parse_line(const char *p, size_t n, uint64_t line_num, const std::unordered_map<std::string, uint64_t> &starts, Chunk &out) {
	if (n == 0 || p[0] == '#') return;
	auto blank = [](char c) { return c == '\t' || c == '\r' || c == ' '; };
	size_t b = 0, e = n;
	while (b < n && blank(p[b])) ++b;
	while (e > b && blank(p[e - 1])) --e;
	// split on tabs; an empty field is dropped (and reported), so the columns after it shift
	std::vector<std::pair<size_t, size_t>> parts;
	char msg[160];
	size_t f = b;
	for (size_t i = b; i < e; ++i) {
		if (p[i] != '\t') continue;
		if (i > f) parts.emplace_back(f, i - f);
		else { snprintf(msg, sizeof(msg), "Unexpected tab delimiter in VCF file, line %llu\n", (unsigned long long) line_num); out.log += msg; }
		f = i + 1;
	}
	if (e > f) parts.emplace_back(f, e - f);
	if (parts.size() < 8) {
		snprintf(msg, sizeof(msg), "Field count < 8 in VCF file, line %llu\n", (unsigned long long) line_num);
		out.log += msg;
		return;
	}
	const std::string chrom(p + parts[0].first, parts[0].second);
	const std::string pos(p + parts[1].first, parts[1].second);
	const char *ref = p + parts[3].first;
	const size_t ref_len = parts[3].second;
	const char *alt = p + parts[4].first;
	const size_t alt_len = parts[4].second;
	auto add = [&](const char *a, size_t an) {
		auto it = starts.find(chrom);
		if (it == starts.end()) {
			out.log += "Chromosome '" + chrom + "' not found in reference but in VCF file, line " + std::to_string(line_num) + "\n";
			return;
		}
		if (an == 1 && a[0] == '.') return;  // missing ALT
		if (!is_sequence(ref, ref_len) || !is_sequence(a, an)) return;
		NgmVariant v;
		v.pos = it->second + (uint64_t) (int64_t) atoi(pos.c_str());
		v.ref_off = (uint32_t) out.seq.size(); v.ref_len = (uint32_t) ref_len; out.seq.append(ref, ref_len);
		v.alt_off = (uint32_t) out.seq.size(); v.alt_len = (uint32_t) an; out.seq.append(a, an);
		out.v.push_back(v);
	};
	// one variant per comma-separated ALT allele; empty alleles are skipped
	size_t s = 0;
	for (size_t i = 0; i <= alt_len; ++i) {
		if (i < alt_len && alt[i] != ',') continue;
		if (i > s) add(alt + s, i - s);
		s = i + 1;
	}
}
}  // namespace

int ngm_vcf_read(const char *path, const std::vector<NgmContig> &contigs, NgmVcf &out) {
	out.v.clear(); out.seq.clear();
	gzFile fp = path ? gzopen(path, "rb") : nullptr;  // (plain files too, like gzopen in VcfParser::open)
	if (!fp) { ngm::pipeline_set_error("Failed to open VCF file %s", path ? path : "(null)"); return -2; }
	std::string data;
	{
		std::vector<char> buf(1 << 22);
		int got;
		while ((got = gzread(fp, buf.data(), (unsigned) buf.size())) > 0) data.append(buf.data(), (size_t) got);
		int zerr = 0;
		const char *zmsg = gzerror(fp, &zerr);
		gzclose(fp);
		if (got < 0 || (zerr != Z_OK && zerr != Z_BUF_ERROR)) { ngm::pipeline_set_error("Failed to read VCF file %s: %s", path, zmsg ? zmsg : "read error"); return -5; }
	}
	// the first contig of a name wins (VcfParser::getRefStart)
	std::unordered_map<std::string, uint64_t> starts;
	for (const NgmContig &c : contigs) starts.emplace(c.name, c.start);
	// line starts, then whole lines to the pool threads; the chunks are joined in file order
	std::vector<size_t> line_at;
	line_at.reserve(data.size() / 64 + 2);
	line_at.push_back(0);
	for (const char *q = data.data(), *end = q + data.size(); (q = (const char *) memchr(q, '\n', (size_t) (end - q))) != nullptr; ++q)
		line_at.push_back((size_t) (q - data.data()) + 1);
	const bool last_open = line_at.back() < data.size();  // a last line without '\n'
	const size_t n_lines = line_at.size() - 1 + (last_open ? 1 : 0);
	if (last_open) line_at.push_back(data.size() + 1);
	const size_t per = 1 << 14;
	const int n_chunks = (int) ((n_lines + per - 1) / per);
	std::vector<Chunk> chunks((size_t) n_chunks);
	ngm::ThreadPool::instance().parallel_for(n_chunks, [&](int lo, int hi) {
		for (int c = lo; c < hi; ++c)
			for (size_t l = (size_t) c * per, e = std::min(n_lines, (size_t) (c + 1) * per); l < e; ++l)
				parse_line(data.data() + line_at[l], line_at[l + 1] - 1 - line_at[l], l + 1, starts, chunks[(size_t) c]);
	}, 1);
	size_t nv = 0, ns = 0;
	for (const Chunk &c : chunks) { nv += c.v.size(); ns += c.seq.size(); }
	if (ns >= 0xFFFFFFFFull) { ngm::pipeline_set_error("VCF file %s: REF/ALT sequences above 4 GB", path); return -27; }
	out.v.reserve(nv); out.seq.reserve(ns);
	for (const Chunk &c : chunks) {
		if (!c.log.empty()) fputs(c.log.c_str(), stderr);
		const uint32_t base = (uint32_t) out.seq.size();
		for (NgmVariant v : c.v) { v.ref_off += base; v.alt_off += base; out.v.push_back(v); }
		out.seq += c.seq;
	}
	return 0;
}

extern "C" {
// host only, no device (tests): the variants of `path` against a contig table as text lines "pos\tREF\tALT\n"; returns the number of
// variants, or a negative error.  *needed: bytes of the text (out may be null to ask for it)
long long ngm_vcf_parse_text(int n_contigs, const char *const *names, const uint64_t *starts, const char *path, char *out, size_t cap, size_t *needed) {
	std::vector<NgmContig> contigs((size_t) std::max(0, n_contigs));
	for (int i = 0; i < n_contigs; ++i) { contigs[i].name = std::string(names[i]).substr(0, 100); contigs[i].start = starts[i]; contigs[i].len = 0; }
	NgmVcf vcf;
	if (int rc = ngm_vcf_read(path, contigs, vcf)) return rc;
	std::string text;
	for (const NgmVariant &v : vcf.v) {
		text += std::to_string(v.pos); text += '\t';
		text.append(vcf.seq, v.ref_off, v.ref_len); text += '\t';
		text.append(vcf.seq, v.alt_off, v.alt_len); text += '\n';
	}
	if (needed) *needed = text.size();
	if (out && cap >= text.size()) memcpy(out, text.data(), text.size());
	return (long long) vcf.v.size();
}
}  // extern "C"
