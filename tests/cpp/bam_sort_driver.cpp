// bam_sort_driver.cpp -- the host-only parts of `ngm-hip --sort` (nextgenmap_amd/csrc/bam_sort.h) for tests/test_bam_sort_host.py, also built
// with -fsanitize=address,undefined:
//   walk IN OUT   IN: chains as [u32 length][bytes].  Every chain is copied into a heap block of exactly its length and walked.  OUT per
//                 chain: u32 accepted, u32 records, u32 notes, u32 message length, the message, then per record of an accepted chain
//                 u64 key, i64 end, u32 bin
//   bai IN OUT    IN: i32 n_ref, u64 n_chunks, u64 n_no_coor, then the arrays of ngm::bamsort::BaiArrays in the order of its members
//                 (u64 each; win_base has n_ref + 1 entries, ioffset win_base[n_ref]).  OUT: the BAI file, then u64 bins
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/bam_sort.h"

namespace bs = ngm::bamsort;

static std::vector<uint8_t> slurp(const char *path) {
	std::vector<uint8_t> v;
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	uint8_t buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}

template <typename T>
static void put(std::string &s, T v) { s.append((const char *) &v, sizeof(T)); }

int main(int argc, char **argv) {
	if (argc != 4) { fprintf(stderr, "usage: bam_sort_driver walk|bai IN OUT\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[2]);
	std::string out;
	if (!strcmp(argv[1], "walk")) {
		size_t at = 0;
		while (at + 4 <= in.size()) {
			uint32_t n;
			memcpy(&n, in.data() + at, 4);
			at += 4;
			if (at + n > in.size()) { fprintf(stderr, "short input\n"); return 2; }
			uint8_t *chain = (uint8_t *) malloc(n ? n : 1);   // exactly the chain: a read past its end is the sanitizer's
			memcpy(chain, in.data() + at, n);
			at += n;
			std::vector<uint32_t> notes;
			uint64_t records = 0;
			std::string err;
			const bool ok = bs::walk(chain, n, &notes, &records, &err);
			put<uint32_t>(out, ok ? 1u : 0u);
			put<uint32_t>(out, (uint32_t) records);
			put<uint32_t>(out, (uint32_t) notes.size());
			put<uint32_t>(out, (uint32_t) err.size());
			out += err;
			if (ok) {
				if (notes.empty() || notes.back() != n || notes.size() != (records + bs::kNoteEvery - 1) / bs::kNoteEvery + 1) { fprintf(stderr, "notes do not cover the chain\n"); return 3; }
				size_t o = 0;
				for (uint64_t i = 0; i < records; ++i) {
					if (i % bs::kNoteEvery == 0 && notes[i / bs::kNoteEvery] != o) { fprintf(stderr, "note %llu is not a record start\n", (unsigned long long) (i / bs::kNoteEvery)); return 3; }
					const uint8_t *p = chain + o;
					const int32_t ref_id = (int32_t) bs::ld32(p + 4), pos = (int32_t) bs::ld32(p + 8);
					const int64_t end = bs::record_end(p);
					put<uint64_t>(out, bs::sort_key(ref_id, pos, bs::ld32(p + 16) >> 16));
					put<int64_t>(out, end);
					put<uint32_t>(out, (pos >= 0 && end <= bs::kMaxEnd) ? bs::reg2bin(pos, end) : 0u);
					o += (size_t) bs::ld32(p) + 4;
				}
				if (o != n) { fprintf(stderr, "the walk did not end at the chain's end\n"); return 3; }
			}
			free(chain);
		}
	} else if (!strcmp(argv[1], "bai")) {
		if (in.size() < 20) return 2;
		int32_t n_ref;
		uint64_t n_chunks, n_no_coor;
		memcpy(&n_ref, in.data(), 4); memcpy(&n_chunks, in.data() + 4, 8); memcpy(&n_no_coor, in.data() + 12, 8);
		std::vector<uint64_t> a((in.size() - 20) / 8);
		memcpy(a.data(), in.data() + 20, a.size() * 8);
		const size_t fixed = 3 * (size_t) n_chunks + 4 * (size_t) n_ref + (size_t) n_ref + 1;
		if (n_ref < 0 || a.size() < fixed || a.size() != fixed + a[fixed - 1]) { fprintf(stderr, "bad array sizes\n"); return 2; }
		bs::BaiArrays A;
		A.n_ref = n_ref; A.n_chunks = (size_t) n_chunks; A.n_no_coor = n_no_coor;
		const uint64_t *p = a.data();
		A.chunk_key = p; p += n_chunks; A.chunk_beg = p; p += n_chunks; A.chunk_end = p; p += n_chunks;
		A.ref_mapped = p; p += n_ref; A.ref_unmapped = p; p += n_ref; A.ref_vbeg = p; p += n_ref; A.ref_vend = p; p += n_ref;
		A.win_base = p; p += n_ref + 1; A.ioffset = p;
		uint64_t bins = 0;
		bs::bai_serialise(A, out, &bins);
		put<uint64_t>(out, bins);
	} else return 2;
	FILE *f = fopen(argv[3], "wb");
	if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
	return 0;
}
