// bam_sort.h -- the host-only parts of `ngm-hip --sort` (csrc/bam_sort.cpp, csrc/bam_sort_device.h): the walk over a run of BAM records that
// validates it before any kernel reads it, the coordinate key, the bin of a region, and the serialiser of the BAI file (SAM specification
// 5.2) from the arrays the device builds.  Compiles with plain g++ (tests/cpp/bam_sort_driver.cpp); the functions marked NGM_BS_HD are the
// ones the kernels run as well.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NGM_BS_HD __host__ __device__
#else
#define NGM_BS_HD
#endif

namespace ngm {
namespace bamsort {

constexpr uint32_t kMember = 0xFF00;       // input bytes of a BGZF member
constexpr uint32_t kNoteEvery = 256;       // the host walk notes the start of every 256th record: one device thread walks each range
constexpr int64_t kMaxEnd = (int64_t) 1 << 29;   // what the bins of a BAI reach
constexpr uint32_t kPseudoBin = 37450;
constexpr size_t kMaxRun = 0xFFFF0000u;    // bytes of one run (32-bit record offsets inside a segment)

NGM_BS_HD inline uint32_t ld32(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24); }

// why a record is refused
enum { kOk = 0, kChain = 1, kBlockSize = 2, kFields = 3 };

// the record at p, `avail` bytes before the end of its run: *size = its bytes including block_size.  Reads the 36 bytes of its fixed part only
// after block_size has said they are there.
NGM_BS_HD inline int check_record(const uint8_t *p, uint64_t avail, uint32_t *size) {
	if (avail < 4) return kChain;
	const uint32_t bs = ld32(p);
	if (bs < 32) return kBlockSize;
	if ((uint64_t) bs + 4 > avail) return kChain;
	const uint64_t l_name = p[12], n_cigar = ld32(p + 16) & 0xFFFFu;
	const int32_t l_seq = (int32_t) ld32(p + 20);
	if (l_seq < 0) return kFields;
	if (l_name + 4 * n_cigar + ((uint64_t) l_seq + 1) / 2 + (uint64_t) l_seq > (uint64_t) bs - 32) return kFields;
	*size = bs + 4;
	return kOk;
}

// samtools' coordinate order: ((uint32) refID, pos + 1, reverse strand) ascending -- refID -1 last; ties keep input order (a stable sort)
NGM_BS_HD inline uint64_t sort_key(int32_t ref_id, int32_t pos, uint32_t flag) {
	return ((uint64_t) (uint32_t) ref_id << 32) | ((uint64_t) (((uint32_t) pos + 1u) & 0x7fffffffu) << 1) | ((flag >> 4) & 1u);
}

// reg2bin (SAM specification 5.3) of [beg, end)
NGM_BS_HD inline uint32_t reg2bin(int64_t beg, int64_t end) {
	--end;
	if ((beg >> 14) == (end >> 14)) return (uint32_t) (4681 + (beg >> 14));
	if ((beg >> 17) == (end >> 17)) return (uint32_t) (585 + (beg >> 17));
	if ((beg >> 20) == (end >> 20)) return (uint32_t) (73 + (beg >> 20));
	if ((beg >> 23) == (end >> 23)) return (uint32_t) (9 + (beg >> 23));
	if ((beg >> 26) == (end >> 26)) return (uint32_t) (1 + (beg >> 26));
	return 0;
}

// end of a record on its reference: pos + the lengths of its M, D, N, = and X operations, pos + 1 without any (p: a record check_record passed)
NGM_BS_HD inline int64_t record_end(const uint8_t *p) {
	const int32_t pos = (int32_t) ld32(p + 8);
	const uint32_t n_cigar = ld32(p + 16) & 0xFFFFu;
	const uint8_t *c = p + 36 + p[12];
	int64_t span = 0;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t v = ld32(c + 4 * (size_t) k), op = v & 15u;
		if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += v >> 4;
	}
	return (int64_t) pos + (span ? span : 1);
}

// The host's walk over a run: every record checked, the chain must end exactly at n.  notes (optional): the offset of every kNoteEvery-th
// record, then n.  err: "record <i> ..." on refusal.
inline bool walk(const uint8_t *p, size_t n, std::vector<uint32_t> *notes, uint64_t *n_records, std::string *err) {
	size_t at = 0;
	uint64_t i = 0;
	char msg[160];
	if (n > kMaxRun) { if (err) *err = "a run holds at most 4 GiB of records"; return false; }
	while (at < n) {
		uint32_t size = 0;
		const int rc = check_record(p + at, n - at, &size);
		if (rc != kOk) {
			if (rc == kChain) snprintf(msg, sizeof(msg), "record %llu at byte %zu does not end inside the run of %zu bytes (the chain of block_size must end exactly there)", (unsigned long long) i, at, n);
			else if (rc == kBlockSize) snprintf(msg, sizeof(msg), "record %llu at byte %zu has block_size %u, below the 32 bytes of a record's fixed part", (unsigned long long) i, at, ld32(p + at));
			else snprintf(msg, sizeof(msg), "record %llu at byte %zu: its name, CIGAR, sequence and qualities exceed its block_size %u", (unsigned long long) i, at, ld32(p + at));
			if (err) *err = msg;
			return false;
		}
		if (notes && i % kNoteEvery == 0) notes->push_back((uint32_t) at);
		at += size;
		++i;
	}
	if (notes) notes->push_back((uint32_t) n);
	if (n_records) *n_records = i;
	return true;
}

// virtual offset of byte u of the sorted uncompressed stream: members of kMember input bytes, C[k] = compressed bytes of members 0..k-1
NGM_BS_HD inline uint64_t virtual_offset(uint64_t u, uint64_t first_member_offset, const uint64_t *C) {
	return ((first_member_offset + C[u / kMember]) << 16) | (u % kMember);
}

// ---- the BAI file from arrays ------------------------------------------------------------------------------------------------------------
struct BaiArrays {
	int n_ref = 0;
	// the chunks, stably sorted by key = reference << 32 | bin: the maximal runs of consecutive records of one reference and bin, in file order
	size_t n_chunks = 0;
	const uint64_t *chunk_key = nullptr, *chunk_beg = nullptr, *chunk_end = nullptr;
	// per reference: records (flag 4 clear / set), virtual offsets of its first record's start and its last record's end
	const uint64_t *ref_mapped = nullptr, *ref_unmapped = nullptr, *ref_vbeg = nullptr, *ref_vend = nullptr;
	// linear index: windows of reference r are ioffset[win_base[r] .. win_base[r + 1])
	const uint64_t *win_base = nullptr, *ioffset = nullptr;
	uint64_t n_no_coor = 0;
};

inline void put_le32(std::string &s, uint32_t v) { char b[4] = {(char) v, (char) (v >> 8), (char) (v >> 16), (char) (v >> 24)}; s.append(b, 4); }
inline void put_le64(std::string &s, uint64_t v) { put_le32(s, (uint32_t) v); put_le32(s, (uint32_t) (v >> 32)); }

inline void bai_serialise(const BaiArrays &a, std::string &out, uint64_t *n_bins) {
	out.clear();
	out.append("BAI\1", 4);
	put_le32(out, (uint32_t) a.n_ref);
	size_t c = 0;
	uint64_t bins = 0;
	for (int r = 0; r < a.n_ref; ++r) {
		const bool any = a.ref_mapped[r] + a.ref_unmapped[r] > 0;
		size_t c1 = c;
		uint32_t n_bin = 0;
		while (c1 < a.n_chunks && (a.chunk_key[c1] >> 32) == (uint64_t) r) { if (c1 == c || a.chunk_key[c1] != a.chunk_key[c1 - 1]) ++n_bin; ++c1; }
		bins += n_bin;
		put_le32(out, n_bin + (any ? 1u : 0u));
		while (c < c1) {
			size_t e = c;
			while (e < c1 && a.chunk_key[e] == a.chunk_key[c]) ++e;
			put_le32(out, (uint32_t) a.chunk_key[c]);
			put_le32(out, (uint32_t) (e - c));
			for (; c < e; ++c) { put_le64(out, a.chunk_beg[c]); put_le64(out, a.chunk_end[c]); }
		}
		if (any) {
			put_le32(out, kPseudoBin);
			put_le32(out, 2);
			put_le64(out, a.ref_vbeg[r]); put_le64(out, a.ref_vend[r]);
			put_le64(out, a.ref_mapped[r]); put_le64(out, a.ref_unmapped[r]);
		}
		const uint64_t w0 = a.win_base[r], w1 = a.win_base[r + 1];
		put_le32(out, (uint32_t) (w1 - w0));
		for (uint64_t w = w0; w < w1; ++w) put_le64(out, a.ioffset[w]);
	}
	put_le64(out, a.n_no_coor);
	if (n_bins) *n_bins = bins;
}

}  // namespace bamsort
}  // namespace ngm
