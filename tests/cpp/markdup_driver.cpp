// markdup_driver.cpp -- the host-only parts of `ngm-hip --sort --markdup` (nextgenmap_amd/csrc/markdup.h) for tests/test_markdup_host.py, also
// built with -fsanitize=address,undefined:
//   markdup_driver IN OUT   IN: chains of whole BAM records as [u32 length][bytes].  Every record is copied into a heap block of exactly its
//                           length (a read past its end is the sanitizer's).  OUT per chain: u32 records; per record u32 examined, i64 u5,
//                           u64 end key, u32 score; then per neighbours g, g + 1: u32 pair_order (0: no pair, 1: the first mate in front, 2: the second),
//                           u64 lo, u64 hi of pair_key(end key g, end key g + 1)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/markdup.h"

namespace bs = ngm::bamsort;
namespace md = ngm::markdup;

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
	if (argc != 3) { fprintf(stderr, "usage: markdup_driver IN OUT\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[1]);
	std::string out;
	size_t at = 0;
	while (at + 4 <= in.size()) {
		uint32_t n;
		memcpy(&n, in.data() + at, 4);
		at += 4;
		if (at + n > in.size()) { fprintf(stderr, "short input\n"); return 2; }
		std::string err;
		uint64_t records = 0;
		if (!bs::walk(in.data() + at, n, nullptr, &records, &err)) { fprintf(stderr, "not a chain of records: %s\n", err.c_str()); return 2; }
		std::vector<uint8_t *> rec;
		for (size_t o = 0; o < n;) {
			const size_t size = (size_t) bs::ld32(in.data() + at + o) + 4;
			uint8_t *p = (uint8_t *) malloc(size);
			memcpy(p, in.data() + at + o, size);
			rec.push_back(p);
			o += size;
		}
		at += n;
		put<uint32_t>(out, (uint32_t) rec.size());
		for (const uint8_t *p : rec) {
			put<uint32_t>(out, md::examined(p) ? 1u : 0u);
			put<int64_t>(out, md::unclipped5(p));
			put<uint64_t>(out, md::end_key_of(p));
			put<uint32_t>(out, md::record_score(p));
		}
		for (size_t g = 0; g + 1 < rec.size(); ++g) {
			uint64_t lo = 0, hi = 0;
			md::pair_key(md::end_key_of(rec[g]), md::end_key_of(rec[g + 1]), &lo, &hi);
			put<uint32_t>(out, (uint32_t) md::pair_order(g > 0 ? rec[g - 1] : nullptr, rec[g], rec[g + 1], g + 2 < rec.size() ? rec[g + 2] : nullptr));
			put<uint64_t>(out, lo);
			put<uint64_t>(out, hi);
		}
		for (uint8_t *p : rec) free(p);
	}
	FILE *f = fopen(argv[2], "wb");
	if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
	return 0;
}
