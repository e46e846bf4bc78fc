// bam_input.h -- SAM and BAM records as reads: what ReadProvider::DetermineParser, SamParser and BamParser do for `ngm -q`.
//
// Host code, header-only (tests/cpp/bam_input_driver.cpp drives it without a GPU).  It works on the whole inflated input in memory
// (BGZF members inflated by the GPU, bgzf_inflate_device.h, or by the host) and hands out views of name, sequence and qualities; from
// there on a record goes the way of a FASTQ record (read_trim.h: -5, the row, --max-polya).
//   format     src/ReadProvider.cpp:480-510   lines that start with '@' are skipped; >= 10 tabs in the first other line: SAM; a leading
//                                             "BAM": BAM; anything else FASTA / FASTQ
//   BAM        src/parser/BamParser.cpp:57-110   every record is a read (parse_all = 1, Config.cpp:489); sequence from the 4-bit codes,
//                                             qualities + 33; flag 0x10: the sequence complemented (upper-case ACGT only) and reversed, the
//                                             qualities reversed
//   SAM        src/parser/SamParser.cpp:89-161   fields 1, 2, 10, 11; '@' lines and empty lines skipped; the same with flag 0x10
// Deliberate differences: a BAM record without qualities (first byte 0xFF) and a SAM '*' are "no quality string", as
// for FASTA; a record with l_seq 0 is the "no sequence" read.
// Nothing here reads outside [p, p + n): every length in a record is checked against the record, every record against the buffer.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

namespace ngm {
namespace bamin {

enum Format { kFastx = 0, kSam = 1, kBam = 2, kUndecided = 3 };

// On the first bytes of the text.  kUndecided: the first line that does not start with '@' is not complete yet and `whole` is false
// (the caller looks again with more text).
inline Format detect(const char *p, size_t n, bool whole) {
	if (n >= 3 && p[0] == 'B' && p[1] == 'A' && p[2] == 'M') return kBam;
	size_t at = 0;
	while (at < n && p[at] == '@') {
		const char *e = (const char *) memchr(p + at, '\n', n - at);
		if (!e) return whole ? kFastx : kUndecided;   // (only '@' lines: whatever reads it finds no record)
		at = (size_t) (e + 1 - p);
	}
	if (at >= n) return whole ? kFastx : kUndecided;
	const char *e = (const char *) memchr(p + at, '\n', n - at);
	if (!e && !whole) return kUndecided;
	const size_t end = e ? (size_t) (e - p) : n;
	int tabs = 0;
	for (size_t i = at; i < end; ++i) tabs += p[i] == '\t';
	return tabs >= 10 ? kSam : kFastx;
}

// the format of a file, plain or gzip (zlib's reader takes both, as the reference's gzopen does)
inline Format detect_file(const char *path) {
	for (size_t cap = (size_t) 1 << 16; cap <= ((size_t) 1 << 30); cap *= 8) {
		gzFile g = gzopen(path, "rb");
		if (!g) return kFastx;
		std::vector<char> buf(cap);
		size_t len = 0;
		int got;
		while (len < cap && (got = gzread(g, buf.data() + len, (unsigned) (cap - len))) > 0) len += (size_t) got;
		gzclose(g);
		const Format f = detect(buf.data(), len, len < cap);
		if (f != kUndecided) return f;
	}
	return kFastx;
}

struct View { const char *name, *seq, *qual; uint32_t name_len, seq_len, qual_len; };

inline char cpl(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

inline uint32_t le32(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24); }

// ---- BAM --------------------------------------------------------------------------------------------------------------
// the offset of the first record (behind the header text and the reference dictionary); 0 with *err set
inline size_t bam_first_record(const uint8_t *p, size_t n, std::string *err) {
	auto bad = [&](const char *m) { if (err) *err = m; return (size_t) 0; };
	if (n < 12 || memcmp(p, "BAM\1", 4) != 0) return bad("BAM input: no BAM\\1 magic");
	const size_t l_text = le32(p + 4);
	if (l_text > n - 12) return bad("BAM input: the header text runs past the end of the file");
	size_t at = 8 + l_text;
	const size_t n_ref = le32(p + at);
	at += 4;
	for (size_t r = 0; r < n_ref; ++r) {
		if (n - at < 4) return bad("BAM input: the reference dictionary runs past the end of the file");
		const size_t l_name = le32(p + at);
		if (l_name > n - at - 4 || n - at - 4 - l_name < 4) return bad("BAM input: the reference dictionary runs past the end of the file");
		at += 4 + l_name + 4;
	}
	return at;
}

// The record at `at`, checked: its size in *size (block_size + 4) and l_seq in *l_seq.  false with *err set for a block_size below 32 or
// past the end (a truncated last record is one), l_read_name 0, or name + CIGAR + sequence + qualities longer than the record.
inline bool bam_check(const uint8_t *p, size_t n, size_t at, size_t *size, uint32_t *l_seq, std::string *err) {
	auto bad = [&](const char *m) { if (err) *err = std::string("BAM input: ") + m + " (record at byte " + std::to_string(at) + " of the inflated file)"; return false; };
	if (n - at < 4) return bad("truncated record");
	const size_t bs = le32(p + at);
	if (bs < 32) return bad("block_size below 32");
	if (bs > n - at - 4) return bad("block_size runs past the end of the file");
	const uint8_t *r = p + at + 4;
	const size_t l_name = r[8], n_cigar = (size_t) r[12] | ((size_t) r[13] << 8), ls = le32(r + 16);
	if (l_name == 0) return bad("l_read_name is 0");
	if (ls > bs) return bad("the sequence is longer than the record");
	if (32 + l_name + 4 * n_cigar + (ls + 1) / 2 + ls > bs) return bad("name, CIGAR, sequence and qualities are longer than the record");
	*size = bs + 4; *l_seq = (uint32_t) ls;
	return true;
}

// every record of the file in order: on_record(offset, size, l_seq).  false with *err set at the first record bam_check refuses
template <typename F>
inline bool bam_walk(const uint8_t *p, size_t n, F on_record, std::string *err) {
	size_t at = bam_first_record(p, n, err);
	if (!at) return false;
	while (at < n) {
		size_t size = 0;
		uint32_t ls = 0;
		if (!bam_check(p, n, at, &size, &ls, err)) return false;
		on_record(at, size, ls);
		at += size;
	}
	return true;
}

// the bytes bam_decode writes at `store` for a record of l_seq bases
inline size_t bam_store_bytes(uint32_t l_seq) { return 2 * (size_t) l_seq; }

// A record bam_check has accepted: the name is a view into the record, sequence and qualities are written at `store`.
inline void bam_decode(const uint8_t *p, size_t at, View &v, char *store) {
	static const char codes[] = "=ACMGRSVTWYHKDBN";
	const uint8_t *r = p + at + 4;
	const size_t l_name = r[8], n_cigar = (size_t) r[12] | ((size_t) r[13] << 8);
	const uint32_t ls = le32(r + 16), flag = (uint32_t) r[14] | ((uint32_t) r[15] << 8);
	const bool reverse = (flag & 0x10u) != 0;
	v.name = (const char *) r + 32;
	v.name_len = (uint32_t) l_name - 1;
	if (v.name_len && memchr(v.name, 0, v.name_len)) v.name_len = (uint32_t) strlen(v.name);   // (the name is a C string inside its field)
	const uint8_t *sq = r + 32 + l_name + 4 * n_cigar, *ql = sq + (ls + 1) / 2;
	char *s = store, *q = store + ls;
	if (!reverse) for (uint32_t i = 0; i < ls; ++i) s[i] = codes[(sq[i >> 1] >> ((i & 1u) ? 0 : 4)) & 15u];
	else for (uint32_t i = 0; i < ls; ++i) s[ls - 1 - i] = cpl(codes[(sq[i >> 1] >> ((i & 1u) ? 0 : 4)) & 15u]);
	v.seq = s; v.seq_len = ls;
	v.qual = q; v.qual_len = 0;
	if (ls && ql[0] != 0xFF) {
		if (!reverse) for (uint32_t i = 0; i < ls; ++i) q[i] = (char) (ql[i] + 33);
		else for (uint32_t i = 0; i < ls; ++i) q[ls - 1 - i] = (char) (ql[i] + 33);
		v.qual_len = ls;
	}
}

// ---- SAM --------------------------------------------------------------------------------------------------------------
// true: the line at `at` is a record ('@' lines and empty lines are not); *next: the start of the line behind it
inline bool sam_is_record(const char *p, size_t n, size_t at, size_t *next) {
	const char *e = (const char *) memchr(p + at, '\n', n - at);
	*next = e ? (size_t) (e + 1 - p) : n;
	return p[at] != '@' && p[at] != '\n';
}

// the bytes sam_decode may write at `store` for the line [at, next)
inline size_t sam_store_bytes(size_t at, size_t next) { return next - at; }

// The record line [at, next).  A line with fewer than 11 fields is the "no sequence" read (SamParser returns 0 for it).  With flag
// 0x10 sequence and qualities are written at `store` (complemented before the row's upper-casing: lower-case bases keep their letter).
// false: the lengths of sequence and qualities differ.
inline bool sam_decode(const char *p, size_t at, size_t next, View &v, char *store) {
	const char *b = p + at, *end = p + next;
	while (end > b && (end[-1] == '\n' || end[-1] == '\r')) --end;
	auto field_end = [&](const char *s) { const char *t = (const char *) memchr(s, '\t', (size_t) (end - s)); return t ? t : end; };
	const char *e = field_end(b);
	v.name = b; v.name_len = (uint32_t) (e - b);
	v.seq = v.qual = e; v.seq_len = v.qual_len = 0;
	if (e == end) return true;
	const char *f = e + 1;
	const bool reverse = (atoi(std::string(f, (size_t) (field_end(f) - f)).c_str()) & 0x10) != 0;
	for (int skip = 0; skip < 8; ++skip) {   // fields 2 .. 9
		f = field_end(f);
		if (f == end) return true;
		++f;
	}
	const char *se = field_end(f);
	const char *sq = f;
	const uint32_t sl = (uint32_t) (se - f);
	if (se == end) return true;   // (no quality field: SamParser returns 0 here too)
	const char *ql = se + 1, *qe = field_end(ql);
	uint32_t qn = (uint32_t) (qe - ql);
	if (qn == 1 && ql[0] == '*') qn = 0;   // no quality string
	else if (qn != sl) return false;
	v.seq = sq; v.seq_len = sl; v.qual = ql; v.qual_len = qn;
	if (reverse) {
		for (uint32_t i = 0; i < sl; ++i) store[sl - 1 - i] = cpl(sq[i]);
		for (uint32_t i = 0; i < qn; ++i) store[sl + qn - 1 - i] = ql[i];
		v.seq = store; v.qual = store + sl;
	}
	return true;
}

}  // namespace bamin
}  // namespace ngm
