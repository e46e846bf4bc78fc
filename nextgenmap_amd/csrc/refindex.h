// refindex.h -- encoded reference + k-mer index, host description shared by the pipeline TUs.
//
// Replaces NextGenMap's _SequenceProvider (src/SequenceProvider.cpp) and CompactPrefixTable
// (src/PrefixTable.cpp).  Coordinates are the reference's: all contigs concatenated, 1000 'N' before the
// first, between and after contigs, every contig starting at an even position (SequenceProvider.cpp:289-326).
//
// HBM layout (MI355X: everything replicated per GPU, 288 GB is plenty for GRCh38):
//   d_genome    : 4-bit symbol classes (A0 C1 G2 T3 N5, the DP kernels' alphabet), 8 bases per dword,
//                 base i in bits 4*(i%8)                                   -- 1.55 GB for GRCh38
//   d_index     : 4^k entries {start, count}: one 8-byte random read per k-mer lookup (the reference reads two
//                 5-byte packed entries, PrefixTable.h:27-61); count is already 0 for k-mers that the reference
//                 treats as unused (>= 9901 occurrences fwd+revcomp, PrefixTable.cpp:468-478)  -- 537 MB
//   d_positions : one uint32 per indexed k-mer occurrence, grouped by k-mer, ascending        -- ~4.1 GB
//                 ... unless the index was built with --vcf (or loaded from a cache `ngm --vcf` wrote): then a list holds its genome
//                 positions in ascending order, then the positions of the variant regions in VCF order (not ascending, a position may
//                 repeat -- regions overlap), then zero slots where the reference's fill pass stored fewer entries than its count pass
//                 reserved (PrefixTable.cpp:360-374 against :411-422; see build_vcf_entries).  What the search makes of them:
//                 * order and repeats: the search kernels and the order replay take a list's entries in index order (the reference's
//                   vote order, CS.cpp:116-160) and identify a bin by its value only; no kernel assumes ascending or distinct positions.
//                 * a zero slot is position 0: `pos - corr` wraps at 2^32 on the GPU where the reference's wraps at 2^64.  With bins of
//                   >= 4 bases (bin_size >= 2) the wrapped bin (2^32 - corr) >> bin_size fits in the kernels' 30 bits and, like the
//                   reference's (2^64 - corr) >> bin_size, lies beyond every genome bin (corr < 1024, the genome below 2^32 - 1024);
//                   bins group the corrections alike in both (2^32 is a multiple of the bin width), so the vote counts, thresholds and
//                   candidate order (rList: first arrival, not hash slot) are the same; such a candidate's window starts past the
//                   genome's end, so both score it against a row of 'N' (ScoreBuffer.cpp:113-118, gather_device.h), which scores at most
//                   0 in local mode: it is never the top score of a mapped read (ScoreBuffer.cpp:418).  Not covered by that argument
//                   and refused with --vcf by ngm-hip: --argos (prints every candidate: the reference converts these positions past its
//                   contig table), -e (negative scores), -n > 1, --bam, several GPUs and shards (not yet tested).
//   d_buckets   : the layout the candidate search actually gathers from: one aligned bucket of W = 4..32 dwords per
//                 k-mer, {count, position 0 .. W-2}, so that a lookup is ONE memory request instead of index entry ->
//                 position list (measured on MI355X, profiles/r02_gather_calibration.txt: random gathers are bound by
//                 ~50 G requests/s whatever their size up to 128 B, where they reach the 6.2 TB/s streaming ceiling).
//                 Lists longer than W-1 keep {count | 1<<31, offset into the position table}; a copy of that table follows the
//                 buckets in the same allocation, so one 32-bit word offset addresses either kind of list.  W from the mean list length
//                 (GRCh38 size: 15.4 -> W = 32, 128 B, 99.98 % of the lists inline)                -- 8.6 GB
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ngm_pipeline.h"
#include "device_mem.h"

namespace ngm {
// std::vector whose resize() leaves new elements uninitialised: the multi-GB host arrays of the reference are filled by all pool
// threads right after they are sized -- value-initialising them first is a second, single-threaded pass over the same memory
template <class T> struct default_init_allocator : std::allocator<T> {
	template <class U> struct rebind { using other = default_init_allocator<U>; };
	template <class U, class... A> void construct(U *p, A &&...a) {
		if constexpr (sizeof...(A) == 0) ::new ((void *) p) U; else ::new ((void *) p) U(std::forward<A>(a)...);
	}
};
using ByteVec = std::vector<uint8_t, default_init_allocator<uint8_t>>;
}  // namespace ngm

struct NgmContig {
	std::string name;
	uint64_t start;  // concatenated coordinate of base 0
	uint64_t len;
};

struct ngm_ref {
	int device = 0;
	ngm_ref_params prm{};
	std::vector<NgmContig> contigs;
	std::vector<uint64_t> start_pos;  // contig starts + one artificial upper bound (SequenceProvider.cpp:370-378)
	uint64_t n_bases = 0;             // nibbles in the encoded genome (binRefIndex after doubling)
	ngm::ByteVec host_cls;            // one class per base (kept for the host-side helpers)
	uint64_t n_entries = 0;
	int auto_max_kfreq = 100;
	bool from_cache = false;          // loaded from NextGenMap's cache files instead of being built
	// device
	ngm::Buf<uint32_t> d_genome;
	uint64_t genome_words = 0;
	ngm::Buf<uint2> d_index;
	ngm::Buf<uint32_t> d_raw_counts;
	ngm::Buf<uint32_t> d_positions;
	ngm::Buf<uint32_t> d_buckets;
	int bucket_log2_words = 2;        // W = 1 << bucket_log2_words dwords per k-mer bucket
	uint32_t bucket_pos_base = 0;     // word offset of the position table copy that follows the buckets in d_buckets
	double overflow_hit_share = 0.0;  // share of all index entries that live in lists longer than W-1
	// canonical buckets (round 3, odd k): ONE bucket per {k-mer, reverse complement} pair -- the search always needs both lists
	// (CS.cpp:116-160), so they live side by side: word 0 = length of the canonical k-mer's list | the other one's << 14 | 1 << 31
	// when the two do not fit, words 1.. = the canonical k-mer's positions followed by its reverse complement's (a pair that does
	// not fit keeps the two list starts in the position table in words 1 and 2).  The canonical one of a pair is the k-mer whose
	// MIDDLE base is A or C (bit 1 of its 2-bit code clear: complementing flips exactly that bit, and the middle base of an odd
	// k-mer stays in the middle), its bucket number the k-mer with that bit removed: a bijection onto [0, 4^k / 2), no table.
	// W = 4..64 dwords from the mean length of both lists (GRCh38 size: 30.8 -> 64 dwords = two 128-byte lines, the second one
	// only read for the ~45 % of the pairs with more than 31 positions).  Same allocation scheme: a copy of the position table
	// follows the buckets.
	ngm::Buf<uint32_t> d_cbuckets;
	int cbucket_log2_words = 2;
	uint32_t cbucket_pos_base = 0;
	// --vcf (PrefixTable.cpp:223-228, :500-574): the variants of the VCF in file order, applied by build_index; and what came of them
	const struct NgmVcf *vcf = nullptr;
	bool vcf_applied = false;
	uint64_t vcf_summary[6] = {0, 0, 0, 0, 0, 0};  // variations loaded, SNPs, indels, ignored, region entries stored, zero slots
	uint64_t vcf_skip_count = 0, vcf_skip_build = 0; // the reference's skipCount / skipBuild (PrefixTable.cpp:439-443)
};

// one variant of a VCF, as VcfParser::add_line keeps it (src/parser/VcfParser.cpp): REF and ALT are ranges of NgmVcf::seq
struct NgmVariant {
	uint64_t pos;  // contig start + POS
	uint32_t ref_off, ref_len, alt_off, alt_len;
};
struct NgmVcf {
	std::vector<NgmVariant> v;
	std::string seq;
};
// reads a plain or gzip VCF against the contig table (0, or a negative error with the reason as the last error); the messages the
// reference logs for odd lines go to stderr, in file order
int ngm_vcf_read(const char *path, const std::vector<NgmContig> &contigs, NgmVcf &out);

// builds the bucket layout `kind` (0: one bucket per k-mer, 1: canonical pairs; odd k only) if it does not exist yet; 0 or -errno
int ngm_ref_ensure_buckets(const ngm_ref *r, int kind);

namespace ngm {
void pipeline_set_error(const char *fmt, ...);
// bam_sort.cpp, for the mapper's SAM stage: the device formatter's records of a batch handed to a sorter on the same device (d_unit_off:
// units + 1 offsets into d_records, the last one n_bytes; both complete), and the device a sorter lives on
int bam_sort_add_device(struct ::ngm_bam_sort *s, uint64_t seq, const void *d_records, size_t n_bytes, const uint32_t *d_unit_off, size_t units);
int bam_sort_device(const struct ::ngm_bam_sort *s);
// for the mapper's SAM stage: a side output (--coverage, --snp, --count, --methyl) as what the four share (side_output.h: its device, the time an
// add kernel of the mapper's took), and per object where such a kernel on its device adds (-22 and the message after the object's finish)
namespace side {
struct Base;
Base *base(struct ::ngm_coverage *c);
Base *base(struct ::ngm_snp *c);
Base *base(struct ::ngm_count *c);
Base *base(struct ::ngm_methyl *c);
}
namespace cov { struct Target { int32_t *counters; const uint64_t *off; int n_ref; unsigned long long *n_aln; }; }   // (off: the contigs' offsets)
namespace snp { struct Target; }                     // snp_device.h
namespace cnt { struct Layout; struct Counters; }    // count.h, count_device.h
namespace met { struct Layout; struct Counters; }    // methyl.h, methyl_device.h
int coverage_target(struct ::ngm_coverage *c, cov::Target *t);
int snp_target(struct ::ngm_snp *c, snp::Target *t);
int count_target(struct ::ngm_count *c, cnt::Layout *l, cnt::Counters *t);
int methyl_target(struct ::ngm_methyl *c, met::Layout *l, met::Counters *t);
// k-mer integer as the reference builds it: 2 bits per base, A0 C1 T2 G3 ((c >> 1) & 3, CSstatic.cpp:20-22)
inline uint32_t kmer_code_of_class(uint32_t cls) { return cls == 2 ? 3u : (cls == 3 ? 2u : cls); }
// reverse complement of a k-mer integer (PrefixTable.cpp:94-108), valid for 2k <= 32
inline uint32_t kmer_revcomp(uint32_t prefix, int k);
// canonical pairs (odd k): bit 2*(k/2)+1 of a k-mer -- the high bit of its middle base -- tells the two k-mers of a pair apart
inline int kmer_canon_bit(int k) { return 2 * (k / 2) + 1; }
inline uint32_t kmer_canon_id(uint32_t canon_kmer, int k) { const int b = kmer_canon_bit(k); return ((canon_kmer >> (b + 1)) << b) | (canon_kmer & ((1u << b) - 1u)); }
inline uint32_t kmer_of_canon_id(uint32_t id, int k) { const int b = kmer_canon_bit(k); return ((id >> b) << (b + 1)) | (id & ((1u << b) - 1u)); }
inline uint32_t kmer_revcomp(uint32_t prefix, int k) {
	const int shift = 32 - 2 * k;
	uint32_t c = (prefix ^ 0xAAAAAAAAu) << shift;
	c = (c & 0xFFFF0000u) >> 16 | (c & 0x0000FFFFu) << 16;
	c = (c & 0xFF00FF00u) >> 8 | (c & 0x00FF00FFu) << 8;
	c = (c & 0xF0F0F0F0u) >> 4 | (c & 0x0F0F0F0Fu) << 4;
	c = (c & 0xCCCCCCCCu) >> 2 | (c & 0x33333333u) << 2;
	return c;
}
}  // namespace ngm
