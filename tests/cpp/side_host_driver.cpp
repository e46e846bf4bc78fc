// side_host_driver.cpp -- what the side outputs share on the host (nextgenmap_amd/csrc/side_host.h) as a stand-alone program, for
// tests/test_side_host.py: plain g++, no GPU; ngm::pipeline_set_error is this file's own and keeps the text.
//   side_host_driver check <fn> <cov|snp> <in>   in: "<n_ref> <n>", n ref_ids, n pos0s, n + 1 CIGAR offsets, the CIGAR text, then the sequence
//                                                offsets (or "NULL"), the sequence text and the quality text; a text is a word, "-" an empty
//                                                one, "NULL" none.  Prints check_batch's return value and the message.
//   side_host_driver take <in> <cap> <0|1>       in: a text of whole lines; one take_whole_lines call with a buffer of exactly cap bytes (1) or
//                                                none (0): prints "<return> <taken>" and the bytes copied.
//   side_host_driver drain <in>                  the same text drained with cap = 1 that grows to what a call asks for: prints the pieces' sizes,
//                                                then the bytes.
//   side_host_driver ref <in>                    in: "<n>", then per contig "<name|NULL> <declared length> <sequence|NULL>": RefView from these
//                                                arrays; prints "ok" with lens, start, the packed words and the name table, or the message.
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/side_host.h"

namespace side = ngm::side;

static char g_error[512] = "";
void ngm::pipeline_set_error(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}

namespace {
struct Text {   // a word of the input: none, or exactly its bytes and a NUL on the heap (so that a read past them is seen)
	bool null = true;
	std::unique_ptr<char[]> p;
	const char *get() const { return null ? nullptr : p.get(); }
};
Text read_text(std::istream &in) {
	std::string w;
	in >> w;
	Text t;
	if (w == "NULL") return t;
	if (w == "-") w.clear();
	t.null = false;
	t.p.reset(new char[w.size() + 1]);
	memcpy(t.p.get(), w.c_str(), w.size() + 1);
	return t;
}
template <typename T> std::vector<T> read_n(std::istream &in, size_t n) {
	std::vector<T> v(n);
	for (T &x : v) { long long y = 0; in >> y; x = (T) y; }
	return v;
}
std::string slurp(const char *path) {
	std::ifstream in(path, std::ios::binary);
	return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}
}  // namespace

int main(int argc, char **argv) {
	if (argc < 3) { fprintf(stderr, "usage: side_host_driver check <fn> <cov|snp> <in> | take <in> <cap> <0|1> | drain <in> | ref <in>\n"); return 2; }
	const std::string mode = argv[1];
	if (mode == "check" && argc == 5) {
		std::ifstream in(argv[4]);
		int n_ref = 0;
		size_t n = 0;
		in >> n_ref >> n;
		const std::vector<int32_t> ref_id = read_n<int32_t>(in, n), pos0 = read_n<int32_t>(in, n);
		const std::vector<uint32_t> cigar_off = read_n<uint32_t>(in, n + 1);
		const Text cigar = read_text(in);
		std::string w;
		std::vector<uint32_t> seq_off;
		in >> w;
		const bool with_seq = w != "NULL";
		if (with_seq) { seq_off = read_n<uint32_t>(in, n); seq_off.insert(seq_off.begin(), (uint32_t) std::stoul(w)); }
		const Text seq = read_text(in), qual = read_text(in);
		if (!in) { fprintf(stderr, "short input\n"); return 2; }
		const bool snp = std::string(argv[3]) == "snp";
		const int rc = side::check_batch(argv[2], cigar_off.data(), cigar.get(), with_seq ? seq_off.data() : nullptr, seq.get(), qual.get(), n, [&](size_t i, const char *cg, uint32_t len, uint64_t seq_len) {
			const int why = snp ? ngm::snp::check_alignment(ref_id[i], pos0[i], cg, len, n_ref, seq_len) : ngm::cov::check_alignment(ref_id[i], pos0[i], cg, len, n_ref);
			return why == ngm::cov::kOk ? nullptr : snp ? ngm::snp::why(why) : ngm::cov::why(why);
		});
		printf("%d\n%s\n", rc, rc ? g_error : "");
		return 0;
	}
	if (mode == "take" && argc == 5) {
		const std::string text = slurp(argv[2]);
		const size_t cap = (size_t) atoll(argv[3]);
		std::vector<char> out(cap);   // (exactly cap bytes: a byte too many is seen)
		size_t taken = 99;
		const long long r = side::take_whole_lines(text.data(), text.size(), argv[4][0] == '1' ? out.data() : nullptr, cap, &taken);
		printf("%lld %zu\n", r, taken);
		if (taken) fwrite(out.data(), 1, taken, stdout);
		return 0;
	}
	if (mode == "drain") {
		const std::string text = slurp(argv[2]);
		std::string got;
		size_t at = 0, cap = 1;
		while (at < text.size()) {
			std::vector<char> out(cap);
			size_t taken = 0;
			const long long r = side::take_whole_lines(text.data() + at, text.size() - at, out.data(), cap, &taken);
			if (r <= 0) { fprintf(stderr, "take_whole_lines gave %lld\n", r); return 1; }
			if ((size_t) r > cap) { if (taken) { fprintf(stderr, "bytes were taken by a call that asks for more room\n"); return 1; } cap = (size_t) r; continue; }
			if ((size_t) r != taken) { fprintf(stderr, "%lld returned, %zu taken\n", r, taken); return 1; }
			printf("%zu ", taken);
			got.append(out.data(), taken);
			at += taken;
		}
		printf("\n%s", got.c_str());
		return 0;
	}
	if (mode == "ref") {
		std::ifstream in(argv[2]);
		size_t n = 0;
		in >> n;
		std::vector<Text> names, seqs;
		std::vector<uint32_t> lens(n);
		for (size_t c = 0; c < n; ++c) { names.push_back(read_text(in)); in >> lens[c]; seqs.push_back(read_text(in)); }
		std::vector<const char *> name_p, seq_p;
		for (size_t c = 0; c < n; ++c) { name_p.push_back(names[c].get()); seq_p.push_back(seqs[c].get()); }
		side::RefView v;
		if (!v.from_arrays("ngm_snp_create", (int) n, lens.data(), name_p.data(), seq_p.data(), true, true)) { printf("refused\n%s\n", g_error); return 0; }
		printf("ok\n");
		for (uint32_t l : v.lens) printf("%u ", l);
		printf("\n");
		for (uint64_t s : v.start) printf("%llu ", (unsigned long long) s);
		printf("\n");
		for (uint32_t x : v.words) printf("%08x ", x);
		std::vector<char> text;
		std::vector<uint32_t> name_off;
		v.name_table(text, name_off);
		printf("\n%s\n", std::string(text.begin(), text.end()).c_str());
		for (uint32_t o : name_off) printf("%u ", o);
		printf("\n");
		return 0;
	}
	fprintf(stderr, "unknown mode\n");
	return 2;
}
