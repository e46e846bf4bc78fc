// cli_format.h -- the host formatter of `ngm-hip`: mapping results -> SAM lines or BAM records, the output filter, the pair writer.
// It is what the GPU writers (csrc/sam_device.h) are compared against, and it is the route of -n > 1, --broken-pairs,
// NGM_HIP_HOST_SAM=1 and NGM_HIP_BAM_HOST_RECORDS=1.  Plain host code: the types of the C ABI, no call into the library -- what it
// needs from outside (reference classes for the SLAM-seq tags, where the --coverage / --snp / --count records go) comes through callbacks.
//   output filter                    src/writer/GenericReadWriter.h:190-254 (min_identity, min_residues), min_mq
//   SAM records                      src/writer/SAMWriter.cpp:98-228, :230-373
//   BAM records                      src/writer/BAMWriter.cpp:147-375, :428-433
//   pair statistics                  src/AlignmentBuffer.cpp:175-199
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ngm_hip.h"
#include "../../include/ngm_pipeline.h"
#include "bam_writer.h"

namespace ngm::cli {

// a read as the pipeline holds it: views into the mapped file (plain FASTQ) or into storage owned by the batch
struct Rec { const char *name; const char *seq; const char *qual; uint32_t name_len, seq_len, qual_len; uint8_t unit; uint16_t polya; };   // seq / qual: behind the -5 prefix; polya: bases --max-polya cut (XA:i); unit: --broken-pairs, see Read

// ---- SAM text, appended to a std::string (no stdio in the hot loop) -----------------------------------------------
inline void put_u64(std::string &s, unsigned long long v) {
	char b[24];
	int i = 24;
	do { b[--i] = (char) ('0' + v % 10); v /= 10; } while (v);
	s.append(b + i, 24 - i);
}
inline void put_i64(std::string &s, long long v) { if (v < 0) { s.push_back('-'); put_u64(s, (unsigned long long) (-(v + 1)) + 1ull); } else put_u64(s, (unsigned long long) v); }
// printf("%g") of roundf(identity * 10000) / 10000 (SAMWriter.cpp:163): at most four decimals, trailing zeros dropped
inline void put_identity(std::string &s, float identity) {
	const float r = roundf(identity * 10000.0f);
	if (!(r >= 0.0f && r <= 10000.0f)) { char b[32]; const int k = snprintf(b, sizeof(b), "%g", r / 10000.0f); s.append(b, k); return; }
	const int iv = (int) r;
	if (iv == 10000) { s.push_back('1'); return; }
	if (iv == 0) { s.push_back('0'); return; }
	char b[6] = {'0', '.', (char) ('0' + iv / 1000), (char) ('0' + iv / 100 % 10), (char) ('0' + iv / 10 % 10), (char) ('0' + iv % 10)};
	int k = 6;
	while (b[k - 1] == '0') --k;
	s.append(b, k);
}

// what one format_range call hands to --coverage, --snp, --count and --methyl: its records without 0x100, as the arrays ngm_coverage_add /
// ngm_snp_add / ngm_count_add / ngm_methyl_add take (rev: flag bit 0x10 of each record; MethylAcc's bottom: its ZS:Z tag begins with '-')
struct CovAcc { std::vector<int32_t> ref, pos; std::vector<uint32_t> off; std::string text; };
struct SnpAcc { std::vector<int32_t> ref, pos; std::vector<uint32_t> off, seq_off; std::vector<uint8_t> rev; std::string text, seq, qual; };
struct MethylAcc : SnpAcc { std::vector<uint8_t> bottom; };

struct HostFormatter {
	// ---- set once per run ----
	float min_identity = 0.65f, min_residues = 0.5f;
	int min_mq = 0, paired = 0, topn = 1, strata = 0, bam = 0, clip = 0 /* --hard-clip or --silent-clip */, no_unal = 0, bs_mapping = 0, slam_seq = 0, variant = 0;
	bool xa_tag = false;   // trimPolyA (SAMWriter.h:11): XA:i on every record, 0 when nothing was cut
	std::string rg_id, rg_mapped, rg_unmapped;   // set_read_group
	std::vector<std::string> contig_names;
	int q = 0;             // bytes per read row
	size_t stride = 0;     // bytes per CIGAR / MD row
	int min_insert = 0, max_insert = 2147483647;
	std::function<void(int contig, uint64_t pos, int span, uint8_t *out)> ref_classes;   // --slam-seq: the classes of `span` reference bases (ngm_ref_host_classes)
	// --coverage / --snp / --count / --methyl: set = wanted.  Called once per range that has such records (snp, count, methyl: once for those
	// without a quality string, once for those with)
	std::function<void(const CovAcc &)> add_coverage;
	std::function<void(const SnpAcc &, bool has_qual)> add_snp, add_count;
	std::function<void(const MethylAcc &, bool has_qual)> add_methyl;

	void set_read_group(const std::string &id) {
		rg_id = id;
		rg_mapped = id.empty() ? std::string() : "RG:Z:" + id + "\t";
		rg_unmapped = id.empty() ? std::string() : "\tRG:Z:" + id;
	}

	// ---- a range of a batch ----
	struct Input { const Rec *recs; const ngm_hit *hits; const char *rows, *cig, *md; };   // hits / cig / md: topn entries per read
	// AlignmentBuffer::WriteRead's pair counters: pairs with both mates mapped, those of them broken, the others' insert sizes
	struct Counts { size_t total = 0, mapped = 0, written = 0; uint64_t pair[3] = {0, 0, 0}; };
	struct View { const Rec *r; const ngm_hit *h; const char *row; int L; const char *cigar, *md; };
	struct BamMate { int ref; long long pos0; long long tlen; };  // what BAMWriter::DoWritePair passes on (0-based, -1 = none; its own TLEN rule)
	struct Side { CovAcc cov; MethylAcc snp[2]; };   // snp[0]: records without a quality string, [1]: with one
	struct SlamTags { int tc = 0; int rates[25] = {0}; std::string mp; };

	View view(const Input &in, int i, int t = 0) const {
		const size_t e = (size_t) i * topn + t;
		View v{&in.recs[i], &in.hits[e], in.rows + (size_t) i * q, 0, &in.cig[e * stride], &in.md[e * stride]};
		v.L = (int) strnlen(v.row, q);
		return v;
	}
	// GenericReadWriter.h:205-215, :262-273: the identity / residue filter (min_residues: a fraction of the read up to 1, a count above)
	bool filter(const View &v) const {
		float min_res = min_residues;
		if (min_res <= 1.0f) min_res = v.L * min_res;
		return v.h->identity >= min_identity && (float) (v.L - v.h->qstart - v.h->qend) >= min_res;
	}
	bool passes(const View &v) const { return v.h->mapped && v.h->mapq >= min_mq && filter(v); }

	static char complement(char ch) { return ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch; }
	// n bases from s0 on of the read as its record prints it (reverse strand: the reverse complement)
	static void oriented_seq(const View &v, int s0, int n, char *dst) {
		if (!v.h->reverse) { if (n > 0) memcpy(dst, v.row + s0, (size_t) n); return; }
		for (int t = 0; t < n; ++t) dst[t] = complement(v.row[v.L - 1 - (s0 + t)]);
	}
	// ... and their qualities: the string as the reference holds it is the first L characters (IParser.h copies qry_max_len - 1 at most).
	// Where it ends before the bases do, pad: ':' for the rest (BAM, --snp), else stop (SAM).  Returns the characters written.
	static int oriented_qual(const View &v, int s0, int n, char *dst, bool pad) {
		const int QL = std::min<int>((int) v.r->qual_len, v.L);
		const int take = std::max(0, std::min(n, QL - s0));
		if (!v.h->reverse) { if (take > 0) memcpy(dst, v.r->qual + s0, (size_t) take); }
		else for (int t = 0; t < take; ++t) dst[t] = v.r->qual[QL - 1 - (s0 + t)];
		if (!pad) return take;
		for (int t = take; t < n; ++t) dst[t] = ':';
		return std::max(n, 0);
	}

	// SLAM-seq tags (SAMWriter.cpp:203-221, GenericReadWriter::computeSlaSeqTags over the per-column records of computeCigarMD,
	// SWOclCigar.cpp:484-540); the device twin is sam_slam_tags (csrc/sam_device.h)
	SlamTags slam_tags(const View &v) const {
		const ngm_hit &h = *v.h;
		auto read_char = [&](int i) -> char { return h.reverse ? complement(v.row[v.L - 1 - i]) : v.row[i]; };
		auto read_class = [](char ch) -> unsigned { return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : ch == 'N' ? 5u : 4u; };
		int span = 0;
		for (const char *c = v.cigar, *e = c + strlen(c); c < e;) { int num = 0; while (c < e && *c >= '0' && *c <= '9') num = num * 10 + (*c++ - '0'); if (c < e) { if (*c == 'M' || *c == 'D') span += num; ++c; } }
		std::vector<uint8_t> refc((size_t) span + 1, 5);
		ref_classes(h.contig, h.pos, span, refc.data());
		SlamTags tg;
		int read_i = h.qstart, ref_i = 0;
		const bool variant_cpu = variant == NGM_VARIANT_OCL_CPU, alt_tables = (slam_seq & 2) != 0;
		for (const char *c = v.cigar, *e = c + strlen(c); c < e;) {
			int num = 0;
			while (c < e && *c >= '0' && *c <= '9') num = num * 10 + (*c++ - '0');
			if (c >= e) break;
			const char op = *c++;
			if (op == 'M') {
				for (int k2 = 0; k2 < num; ++k2) {
					const unsigned fc = refc[ref_i + k2];
					const char rch = read_char(read_i + k2);
					const unsigned rc = read_class(rch);
					const int type = 5 * (int) (fc <= 3u ? fc : 4u) + (int) (rc <= 3u ? rc : 4u);
					tg.rates[type] += 1;
					const char fch = fc == 0u ? 'A' : fc == 1u ? 'C' : fc == 2u ? 'G' : fc == 3u ? 'T' : fc == 4u ? 'x' : 'N';
					const bool eq = !variant_cpu ? (rch == fch) : (alt_tables ? rc == fc : (rc <= 3u && rc == fc));
					if (!eq) { if (!tg.mp.empty()) tg.mp.push_back(','); put_i64(tg.mp, type); tg.mp.push_back(':'); put_i64(tg.mp, read_i + k2 + 1); tg.mp.push_back(':'); put_i64(tg.mp, ref_i + k2 + 1); }
				}
				read_i += num; ref_i += num;
			} else if (op == 'I') read_i += num;
			else if (op == 'D') ref_i += num;
		}
		tg.tc = h.reverse ? tg.rates[0 * 5 + 2] : tg.rates[3 * 5 + 1];
		return tg;
	}
	// the 25 counts of RA:Z: the SAM writer joins them with commas, the BAM writer follows every one with a comma (BAMWriter.cpp:273-292)
	static std::string slam_ra(const SlamTags &tg, bool trailing_comma) {
		std::string ra;
		for (int i = 0; i < 25; ++i) { if (i) ra.push_back(','); put_i64(ra, tg.rates[i]); }
		if (trailing_comma) ra.push_back(',');
		return ra;
	}
	// SAMWriter.cpp:173-187: first mates / single reads "++" or "-+", second mates "--" or "+-"
	const char *zs_tag(const ngm_hit &h, int flags) const { return (paired && (flags & 0x80)) ? (h.reverse ? "+-" : "--") : (h.reverse ? "-+" : "++"); }

	// SAMWriter::DoWriteReadGeneric (SAMWriter.cpp:98-228), BAMWriter::DoWriteReadGeneric (BAMWriter.cpp:147-298)
	void write_mapped(std::string &s, Counts &c, Side *side, const View &v, int flags, const char *rnext, unsigned long long pnext, long long tlen, const BamMate &bm) const {
		const ngm_hit &h = *v.h;
		const int L = v.L;
		const bool noq = v.r->qual_len == 0;
		if (h.reverse) flags |= 0x10;
		const int s0 = clip ? h.qstart : 0, sl = std::max(0, clip ? L - h.qstart - h.qend : L);
		if (side && add_coverage && !(flags & 0x100)) {
			CovAcc &a = side->cov;
			a.ref.push_back(h.contig); a.pos.push_back((int32_t) h.pos); a.off.push_back((uint32_t) a.text.size());
			a.text += v.cigar;
		}
		if (side && (add_snp || add_count || add_methyl) && !(flags & 0x100)) {   // the sequence and the qualities as the record prints them
			MethylAcc &a = side->snp[noq ? 0 : 1];
			a.ref.push_back(h.contig); a.pos.push_back((int32_t) h.pos); a.off.push_back((uint32_t) a.text.size()); a.seq_off.push_back((uint32_t) a.seq.size());
			a.rev.push_back(h.reverse ? 1 : 0);
			if (add_methyl) a.bottom.push_back(zs_tag(h, flags)[0] == '-' ? 1 : 0);
			a.text += v.cigar;
			a.seq.resize(a.seq.size() + sl);
			oriented_seq(v, s0, sl, &a.seq[a.seq.size() - sl]);
			if (!noq) { a.qual.resize(a.qual.size() + sl); (void) oriented_qual(v, s0, sl, &a.qual[a.qual.size() - sl], true); }
		}
		if (bam) {
			char seq[1024], qual[1024];
			const int n = std::min(sl, 1000);
			oriented_seq(v, s0, n, seq);
			(void) oriented_qual(v, s0, n, qual, true);
			ngm::bam::Tags tg;
			tg.add_int("AS", (int) h.score); tg.add_int("NM", h.nm); tg.add_int("NH", h.n_best);
			if (bs_mapping) tg.add_string("ZS", zs_tag(h, flags), 2);  // BAMWriter.cpp:240-254
			tg.add_float("XI", roundf(h.identity * 10000.0f) / 10000.0f);
			if (xa_tag) tg.add_int("XA", v.r->polya);   // BAMWriter.cpp:258-260
			tg.add_int("X0", h.n_best); tg.add_int("XE", (int) h.max_votes); tg.add_int("XR", L - h.qstart - h.qend);
			tg.add_string("MD", v.md, strlen(v.md));
			if (!rg_id.empty()) tg.add_string("RG", rg_id.data(), rg_id.size());
			if (slam_seq) {   // TC:i, RA:Z, MP:Z when there are mismatches
				const SlamTags st = slam_tags(v);
				const std::string ra = slam_ra(st, true);
				tg.add_int("TC", st.tc);
				tg.add_string("RA", ra.data(), ra.size());
				if (!st.mp.empty()) tg.add_string("MP", st.mp.data(), st.mp.size());
			}
			ngm::bam::put_record(s, v.r->name, v.r->name_len, (uint32_t) flags, h.contig, (int) h.pos, h.mapq, v.cigar, seq, (size_t) n, noq ? nullptr : qual,
					bm.ref, (int) bm.pos0, (int) bm.tlen, tg);
			++c.written;
			return;
		}
		s.append(v.r->name, v.r->name_len); s.push_back('\t'); put_u64(s, (unsigned) flags); s.push_back('\t');
		s += contig_names[h.contig]; s.push_back('\t'); put_u64(s, (unsigned long long) h.pos + 1); s.push_back('\t'); put_i64(s, h.mapq); s.push_back('\t');
		s += v.cigar; s.push_back('\t'); s += rnext; s.push_back('\t'); put_u64(s, pnext); s.push_back('\t'); put_i64(s, tlen); s.push_back('\t');
		const size_t at = s.size();
		s.resize(at + sl);
		oriented_seq(v, s0, sl, &s[at]);
		s.push_back('\t');
		if (noq) s.push_back('*');
		else {
			const size_t aq = s.size();
			s.resize(aq + sl);
			s.resize(aq + oriented_qual(v, s0, sl, &s[aq], false));
		}
		s.push_back('\t');
		s += rg_mapped;
		s += "AS:i:"; put_i64(s, (int) h.score); s += "\tNM:i:"; put_i64(s, h.nm); s += "\tNH:i:"; put_i64(s, h.n_best);
		if (bs_mapping) { s += "\tZS:Z:"; s += zs_tag(h, flags); }
		s += "\tXI:f:"; put_identity(s, h.identity);
		s += "\tX0:i:"; put_i64(s, h.n_best);
		if (xa_tag) { s += "\tXA:i:"; put_i64(s, v.r->polya); }   // SAMWriter.cpp:192-194
		s += "\tXE:i:"; put_i64(s, (int) h.max_votes); s += "\tXR:i:"; put_i64(s, L - h.qstart - h.qend); s += "\tMD:Z:"; s += v.md;
		if (slam_seq) {
			const SlamTags st = slam_tags(v);
			s += "\tTC:i:"; put_i64(s, st.tc); s += "\tRA:Z:"; s += slam_ra(st, false);
			if (!st.mp.empty()) { s += "\tMP:Z:"; s += st.mp; }
		}
		s.push_back('\n');
		++c.written;
	}
	// SAMWriter::DoWriteUnmappedReadGeneric (SAMWriter.cpp:311-372): contig < 0 prints '*'
	void write_unmapped(std::string &s, Counts &c, const View &v, int flags, int contig, unsigned long long pos1, char rnext, unsigned long long pnext1) const {
		if (no_unal) return;
		const bool noq = v.r->qual_len == 0;
		if (bam) {  // BAMWriter::DoWriteUnmappedReadGeneric (BAMWriter.cpp:300-375): reference / mate fields = the mapped mate's, 0-based
			char qual[1024];
			const int n = std::min(v.L, 1000), QL = std::min<int>((int) v.r->qual_len, v.L);
			for (int t = 0; t < n; ++t) qual[t] = t < QL ? v.r->qual[t] : ':';
			ngm::bam::Tags tg;
			if (xa_tag) tg.add_int("XA", v.r->polya);   // BAMWriter.cpp:356-358
			if (!rg_id.empty()) tg.add_string("RG", rg_id.data(), rg_id.size());
			const int p0 = contig >= 0 ? (int) pos1 - 1 : -1;
			ngm::bam::put_record(s, v.r->name, v.r->name_len, (uint32_t) (flags | 0x4), contig >= 0 ? contig : -1, p0, 0, nullptr, v.row, (size_t) n,
					noq ? nullptr : qual, contig >= 0 ? contig : -1, p0, 0, tg);
			++c.written;
			return;
		}
		s.append(v.r->name, v.r->name_len); s.push_back('\t'); put_u64(s, (unsigned) (flags | 0x4)); s.push_back('\t');
		if (contig >= 0) s += contig_names[contig]; else s.push_back('*');
		s.push_back('\t'); put_u64(s, pos1); s += "\t0\t*\t"; s.push_back(rnext); s.push_back('\t'); put_u64(s, pnext1); s += "\t0\t";
		s.append(v.row, v.L); s.push_back('\t');
		if (noq) s.push_back('*'); else s.append(v.r->qual, std::min<int>((int) v.r->qual_len, v.L));
		if (xa_tag) { s += "\tXA:i:"; put_i64(s, v.r->polya); }   // SAMWriter.cpp:355-357
		s += rg_unmapped;
		s.push_back('\n');
		++c.written;
	}
	// a read on its own (single-end with one alignment per read; --broken-pairs: a read without its mate)
	void write_single(std::string &s, Counts &c, Side *side, const View &v) const {
		++c.total;
		if (!passes(v)) { write_unmapped(s, c, v, 0, -1, 0, '*', 0); return; }
		++c.mapped;
		write_mapped(s, c, side, v, 0, "*", 0, 0, BamMate{-1, -1, 0});
	}
	void format_single_end(const Input &in, int lo, int hi, std::string &s, Counts &c, Side *side) const {
		std::vector<std::tuple<int, unsigned long long, int>> seen;
		for (int i = lo; i < hi; ++i) {
			const View v = view(in, i);
			if (v.r->seq_len == 0) continue;  // NGMNames::Empty reads are discarded (GenericReadWriter.h:245-247)
			if (topn == 1) { write_single(s, c, side, v); continue; }
			++c.total;
			// GenericReadWriter::WriteRead with several alignments (GenericReadWriter.h:199-243) behind AlignmentBuffer::WriteRead
			// (AlignmentBuffer.cpp:165-175), as the reference does it -- quirks included, because on a repeat-rich genome they decide records
			// (tests/test_gpu_humanlike.py): `mapped` starts as the answer of the LAST alignment's coordinate conversion ("TODO: fix for
			// -n > 1" there), and the identity / residue filter is sticky: once an alignment fails it, no later one is written either.
			// One record per distinct location, 0x100 on all but candidate 0.
			const ngm_hit &h0 = *v.h;
			const int calc = strata ? (h0.n_best <= topn ? h0.n_best : 0) : std::min(h0.n_candidates, topn);   // read->Calculated (ScoreBuffer::topNSE)
			bool mapped = calc > 0 && h0.mapq >= min_mq && view(in, i, calc - 1).h->mapped;   // (AlignmentBuffer.cpp:47: the read's MAPQ against min_mq)
			bool once = false;
			seen.clear();
			for (int t = 0; t < calc && mapped; ++t) {
				const View vt = view(in, i, t);
				mapped = filter(vt);
				if (!mapped) break;
				once = true;
				if (!vt.h->mapped) continue;   // (its position did not convert: the reference would print an unconverted location here -- not mirrored)
				const auto key = std::make_tuple(vt.h->contig, (unsigned long long) vt.h->pos, vt.h->reverse);
				if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
				seen.push_back(key);
				write_mapped(s, c, side, vt, t ? 0x100 : 0, "*", 0, 0, BamMate{-1, -1, 0});
			}
			if (once) ++c.mapped; else write_unmapped(s, c, v, 0, -1, 0, '*', 0);
		}
	}
	void format_pairs(const Input &in, int lo, int hi, std::string &s, Counts &c, Side *side) const {
		for (int i = lo; i + 1 < hi; i += 2) {
			// read1 = the first mate (even ReadId), written second by AlignmentBuffer::WriteRead; read2 = its mate
			const View v1 = view(in, i), v2 = view(in, i + 1);
			if (v2.r->unit & 2) {
				// --broken-pairs: a read without its mate goes out like a single-end read (AlignmentBuffer.cpp:201-203, GenericReadWriter::WriteRead)
				if (v1.r->seq_len != 0) write_single(s, c, side, v1);
				continue;
			}
			if (v1.r->seq_len == 0 || v2.r->seq_len == 0) continue;  // GenericReadWriter.h:250-252
			const ngm_hit &h1 = *v1.h, &h2 = *v2.h;
			if ((h1.pair_flags | h2.pair_flags) & NGM_PAIR_LOST) continue;   // the reference never writes this pair (ngm_mapper_set_reference_score_buffer)
			c.total += 2;
			// AlignmentBuffer::WriteRead (AlignmentBuffer.cpp:175-199): is the pair consistent?
			bool paired_fail = (h1.pair_flags & NGM_PAIR_FAILED) || (h2.pair_flags & NGM_PAIR_FAILED);
			if (h1.mapped && h2.mapped) {
				const long long distance = (h2.pos > h1.pos) ? (long long) (h2.pos - h1.pos) + v1.L : (long long) (h1.pos - h2.pos) + v2.L;
				++c.pair[0];
				if (h1.contig != h2.contig || distance < min_insert || distance > max_insert || h1.reverse == h2.reverse) { paired_fail = true; ++c.pair[1]; }
				else c.pair[2] += (uint64_t) distance;
			}
			const bool m1 = passes(v1), m2 = passes(v2);  // GenericReadWriter::WritePair
			c.mapped += (m1 ? 1 : 0) + (m2 ? 1 : 0);
			const bool swp = (v1.r->unit & 4) != 0;   // (--broken-pairs: the reference's read ids have lost their parity, see the reader)
			const int f1 = 0x1 | (swp ? 0x80 : 0x40), f2 = 0x1 | (swp ? 0x40 : 0x80);  // SAMWriter::DoWritePair (SAMWriter.cpp:230-310)
			const unsigned long long p1 = h1.pos + 1, p2 = h2.pos + 1;
			if (!m1 && !m2) {
				write_unmapped(s, c, v2, f2 | 0x8, -1, 0, '*', 0);
				write_unmapped(s, c, v1, f1 | 0x8, -1, 0, '*', 0);
			} else if (!m1) {
				write_mapped(s, c, side, v2, f2 | 0x8, "=", p2, 0, BamMate{h2.contig, (long long) h2.pos, 0});
				write_unmapped(s, c, v1, f1, h2.contig, p2, '=', p2);
			} else if (!m2) {
				write_unmapped(s, c, v2, f2, h1.contig, p1, '=', p1);
				write_mapped(s, c, side, v1, f1 | 0x8, "=", p1, 0, BamMate{h1.contig, (long long) h1.pos, 0});
			} else if (!paired_fail) {
				if (!h1.reverse) {
					const long long d = ((long long) h2.pos + v2.L - h2.qstart - h2.qend) - (long long) h1.pos;
					const long long db = (long long) h2.pos + v2.L - (long long) h1.pos;  // BAMWriter.cpp:428-433: the whole read length
					write_mapped(s, c, side, v2, f2 | 0x2, "=", p1, -d, BamMate{h2.contig, (long long) h1.pos, -db});
					write_mapped(s, c, side, v1, f1 | 0x2 | 0x20, "=", p2, d, BamMate{h2.contig, (long long) h2.pos, db});
				} else if (!h2.reverse) {
					const long long d = ((long long) h1.pos + v1.L - h1.qstart - h1.qend) - (long long) h2.pos;
					const long long db = (long long) h1.pos + v1.L - (long long) h2.pos;
					write_mapped(s, c, side, v2, f2 | 0x2 | 0x20, "=", p1, d, BamMate{h2.contig, (long long) h1.pos, db});
					write_mapped(s, c, side, v1, f1 | 0x2, "=", p2, -d, BamMate{h2.contig, (long long) h2.pos, -db});
				}
			} else {
				write_mapped(s, c, side, v2, f2 | (h1.reverse ? 0x20 : 0), contig_names[h1.contig].c_str(), p1, 0, BamMate{h1.contig, (long long) h1.pos, 0});
				write_mapped(s, c, side, v1, f1 | (h2.reverse ? 0x20 : 0), contig_names[h2.contig].c_str(), p2, 0, BamMate{h2.contig, (long long) h2.pos, 0});
			}
		}
	}
	// records [lo, hi) of a batch (paired: lo and hi even) -> SAM text or BAM records appended to s, the counters added to c; the range's
	// records without 0x100 go to --coverage, --snp, --count and --methyl in one call each when the range is done
	void format_range(const Input &in, int lo, int hi, std::string &s, Counts &c) const {
		Side side;
		Side *sp = (add_coverage || add_snp || add_count || add_methyl) ? &side : nullptr;
		s.reserve((size_t) (hi - lo) * (size_t) (2 * q + 160));
		if (paired) format_pairs(in, lo, hi, s, c, sp); else format_single_end(in, lo, hi, s, c, sp);
		for (int k = 0; (add_snp || add_count || add_methyl) && k < 2; ++k) {
			MethylAcc &a = side.snp[k];
			if (a.ref.empty()) continue;
			a.off.push_back((uint32_t) a.text.size()); a.seq_off.push_back((uint32_t) a.seq.size());
			if (add_snp) add_snp(a, k == 1);
			if (add_count) add_count(a, k == 1);
			if (add_methyl) add_methyl(a, k == 1);
		}
		if (add_coverage && !side.cov.ref.empty()) {
			side.cov.off.push_back((uint32_t) side.cov.text.size());
			add_coverage(side.cov);
		}
	}
};

}  // namespace ngm::cli
