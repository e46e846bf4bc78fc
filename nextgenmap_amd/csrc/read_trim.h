// read_trim.h -- how a FASTA / FASTQ record becomes the read that is mapped: -5/--trim5, the parser's row, --max-polya.
//
// Host code, header-only (tests/cpp/read_trim_driver.cpp drives it without a GPU).  The device derives a read's length from its
// NUL-padded row, so a row that arrives trimmed needs nothing new in search, score, align or selection; the writers print the
// first `length` quality characters of the string that starts behind the -5 prefix.
//   -5 N          src/parser/IParser.h:70-100     the read is seq[N ..), the quality string qual[N ..); a sequence of N bases or fewer
//                                                 is the "no sequence" read (one 'N', NGMNames::Empty, discarded by the writers)
//   the row       src/parser/IParser.h:69-84      upper-case, non-ACGT -> 'N', at most qry_max_len - 1 bases, NUL-padded
//   --max-polya M src/ReadProvider.cpp:428-443    after all of the above: a tail of more than M 'A' is cut off (an 'N' ends the tail),
//                                                 the number of bases cut is the record's XA:i tag
// The estimation pass (src/ReadProvider.cpp:204-304) reads through the parser only: it sees lengths after -5 and before --max-polya.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ngm {
namespace trim {

struct Options {
	int trim5 = 0;        // Default(TRIM5, 0)
	int max_polya = -1;   // Default(MAX_POLYA, -1): no poly-A trimming, no XA:i tag
};

// -5: the views move behind the prefix.  seq_len 0 afterwards = no sequence; qual_len 0 = no quality string ('*')
inline void trim5(int n5, const char *&seq, uint32_t &seq_len, const char *&qual, uint32_t &qual_len) {
	if (n5 <= 0) return;
	if (seq_len > (uint32_t) n5) { seq += n5; seq_len -= (uint32_t) n5; } else seq_len = 0;
	if (qual_len > (uint32_t) n5) { qual += n5; qual_len -= (uint32_t) n5; } else qual_len = 0;
}

// read->length as the estimation pass sees it for a record with raw_len > 0 bases (parsed with qry_max_len 10 000): a record the
// prefix swallows is the one-base "no sequence" read, and counts as such
inline size_t estimate_len(size_t raw_len, int n5) {
	const size_t n = n5 > 0 ? (size_t) n5 : 0;
	return raw_len > n ? (raw_len - n < 9999 ? raw_len - n : 9999) : 1;
}

// the parser's row of q = qry_max_len bytes; returns the read's length (1 for the "no sequence" read)
inline int pack_row(const char *seq, size_t len, int q, char *row) {
	memset(row, 0, (size_t) q);
	if (len == 0) { row[0] = 'N'; return 1; }
	const int L = (int) (len < (size_t) q - 1 ? len : (size_t) q - 1);
	for (int i = 0; i < L; ++i) {
		const char c = (char) (seq[i] & 0xDF);  // toupper for letters
		row[i] = (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : 'N';
	}
	return L;
}

// --max-polya on a packed row of length L: returns the number of bases cut (0: the tail is max_polya or shorter and stays).  The row
// may come out empty (all NUL): such a read has no candidates and is written as an unmapped record, not discarded
inline int trim_polya(char *row, int L, int max_polya) {
	if (max_polya < 0) return 0;
	int n = 0;
	while (n < L && row[L - 1 - n] == 'A') ++n;
	if (n <= max_polya) return 0;
	memset(row + (L - n), 0, (size_t) n);
	return n;
}

// one record on every input route: moves the views behind the -5 prefix, fills the row, returns polyATrimmed
inline int parse_read(const Options &t, int q, const char *&seq, uint32_t &seq_len, const char *&qual, uint32_t &qual_len, char *row) {
	trim5(t.trim5, seq, seq_len, qual, qual_len);
	const int L = pack_row(seq, seq_len, q, row);
	return trim_polya(row, L, t.max_polya);
}

}  // namespace trim
}  // namespace ngm
