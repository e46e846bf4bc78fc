// side_host.h -- the host-only parts the run-long side outputs (csrc/coverage.cpp, csrc/snp.cpp, csrc/count.cpp, csrc/methyl.cpp) share: the checks in
// front of an add, the whole-lines rule of a text output's next, and the contigs' table of an object.  No HIP here: compiles with plain
// g++ (tests/cpp/side_host_driver.cpp, which supplies its own ngm::pipeline_set_error).  The HIP part: csrc/side_output.h.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "snp.h"

namespace ngm {
void pipeline_set_error(const char *fmt, ...);   // (refindex.cpp; the text ngm_pipeline_last_error() hands out)

namespace side {

// the front of ngm_*_add, over the caller's memory (no lock, nothing on the device yet): the offsets ascend, every alignment passes the
// object's own check -- verdict(i, cigar, cigar_len, seq_len) gives null or why not -- and a quality text, a C string under the sequence's
// offsets, ends where the sequences end.  fn: the function the messages name.  seq_off, seq_text and qual_text may be null.  0 or -22.
template <typename Verdict>
inline int check_batch(const char *fn, const uint32_t *cigar_off, const char *cigar_text, const uint32_t *seq_off, const char *seq_text, const char *qual_text, size_t n, Verdict verdict) {
	const size_t qual_len = qual_text ? strlen(qual_text) : 0;
	for (size_t i = 0; i < n; ++i) {
		if (cigar_off[i + 1] < cigar_off[i] || (cigar_off[i + 1] > cigar_off[i] && !cigar_text)) { pipeline_set_error("%s: alignment %zu: its CIGAR offsets do not ascend", fn, i); return -22; }
		if (seq_off && (seq_off[i + 1] < seq_off[i] || (seq_off[i + 1] > seq_off[i] && !seq_text))) { pipeline_set_error("%s: alignment %zu: its sequence offsets do not ascend", fn, i); return -22; }
		const char *why = verdict(i, cigar_text ? cigar_text + cigar_off[i] : nullptr, cigar_off[i + 1] - cigar_off[i], seq_off ? (uint64_t) (seq_off[i + 1] - seq_off[i]) : 0);
		if (why) { pipeline_set_error("%s: alignment %zu: %s", fn, i, why); return -22; }
		// (the first alignment the quality text does not reach is the one refused)
		if (qual_text && (size_t) seq_off[i + 1] > qual_len) { pipeline_set_error("%s: alignment %zu: %s", fn, i, snp::why(snp::kQualLength)); return -22; }
	}
	if (qual_text && qual_len != (size_t) seq_off[n]) { pipeline_set_error("%s: alignment %zu: %s", fn, n - 1, snp::why(snp::kQualLength)); return -22; }
	return 0;
}

// the tail of ngm_*_next over the left bytes at p (whole lines): as many lines as fit into out are copied and *taken says how many bytes;
// with no out, or a cap below the first line, the size of the first line comes back and nothing is taken
inline long long take_whole_lines(const char *p, size_t left, void *out, size_t cap, size_t *taken) {
	*taken = 0;
	size_t take = std::min(left, cap);
	while (take > 0 && p[take - 1] != '\n') --take;
	if (take == 0 || !out) return (long long) ((const char *) memchr(p, '\n', left) - p + 1);
	memcpy(out, p, take);
	*taken = take;
	return (long long) take;
}

// the contigs of an object: lengths, names, and where each begins in the packed reference (start[n_ref]: its end)
struct RefView {
	std::vector<uint32_t> lens;
	std::vector<const char *> names;
	std::vector<uint64_t> start;
	std::vector<uint32_t> words;   // the packed reference, from the caller's sequences only
	int n_ref() const { return (int) lens.size(); }

	// from the caller's arrays: a contig without a name is refused where need_names says so; with_seq: the sequences are checked and packed
	bool from_arrays(const char *fn, int n, const uint32_t *ref_len, const char *const *ref_name, const char *const *ref_seq, bool need_names, bool with_seq) {
		for (int c = 0; c < n; ++c) {
			if (need_names && !ref_name[c]) { pipeline_set_error("%s: contig %d has no name", fn, c); return false; }
			if (with_seq && (!ref_seq[c] || strnlen(ref_seq[c], (size_t) ref_len[c]) != (size_t) ref_len[c])) { pipeline_set_error("%s: the sequence of contig %d is shorter than its length", fn, c); return false; }
		}
		lens.assign(ref_len, ref_len + n);
		names.assign(ref_name, ref_name + n);
		if (with_seq) words = snp::pack_reference(ref_seq, ref_len, n, start);
		return true;
	}
	// from a resident reference (refindex.h's ngm_ref: contigs with name, start and len; genome_words dwords of 8 bases)
	template <typename Ref>
	bool from_ref(const char *fn, const Ref &r) {
		const size_t n = r.contigs.size();
		lens.resize(n); names.resize(n); start.assign(n + 1, 0);
		for (size_t c = 0; c < n; ++c) {
			if (r.contigs[c].len > 0xffffffffull || r.contigs[c].start + r.contigs[c].len > r.genome_words * 8ull) { pipeline_set_error("%s: contig %d does not fit", fn, (int) c); return false; }
			lens[c] = (uint32_t) r.contigs[c].len; names[c] = r.contigs[c].name.c_str(); start[c] = r.contigs[c].start;
		}
		start[n] = r.genome_words * 8ull;
		return true;
	}
	// the names one behind the other, and where each begins
	void name_table(std::vector<char> &text, std::vector<uint32_t> &name_off) const {
		text.clear();
		name_off.assign(names.size() + 1, 0);
		for (size_t k = 0; k < names.size(); ++k) { text.insert(text.end(), names[k], names[k] + strlen(names[k])); name_off[k + 1] = (uint32_t) text.size(); }
	}
};

}  // namespace side
}  // namespace ngm
