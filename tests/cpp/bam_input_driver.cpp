// bam_input_driver.cpp -- test driver (no GPU): the inflate core of nextgenmap_amd/csrc/bgzf_inflate_device.h and the record code of
// nextgenmap_amd/csrc/bam_input.h, run on the CPU.  The kernel's cooperative steps are loops over the thread index here; the text
// stage of a member is a heap block of exactly ISIZE bytes and the input a heap block of exactly its size, so that a sanitizer build
// sees every access the decoder makes outside them.
//   inflate <members> <out>   the text of a run of BGZF members.  exit 0: written; exit 3: refused ("member <i> status <s>" on stdout,
//                             member -1: the host's walk over the chain refused the data)
//   cases <in> <out>          many runs in one process.  in: [u32 n][n bytes] ...; out: [u32 status][u32 n][n bytes of text] ...
//                             (status 0: inflated; 100: the walk refused; else the Status of the first refused member)
//   detect <file>             prints fastx, sam or bam (file plain or gzip)
//   records <text> <out>      <text>: an inflated BAM or a SAM.  out: one line per read, name TAB sequence TAB qualities ('*': none).
//                             exit 3 with the message on stderr for a damaged record
//   index <text> <step>       BAM: prints the offset of every step-th record, then the number of records
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nextgenmap_amd/csrc/bam_input.h"
#include "../../nextgenmap_amd/csrc/bgzf_inflate_device.h"

namespace inf = ngm::inflate;
namespace bi = ngm::bamin;

static bool read_file(const char *path, std::vector<char> &v) {
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	char buf[65536];
	size_t k;
	while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return true;
}

// what the kernel does for a run of members; returns 0, 100 (walk) or the first refused member's status
static uint32_t inflate_run(const char *data, size_t n, std::string &text, long long *bad_member) {
	static const std::vector<uint32_t> tab = inf::crc_tables();   // (the tables the kernel gets: bgzf.cpp uploads the same vector)
	*bad_member = -1;
	uint8_t *in = (uint8_t *) malloc(n ? n : 1);   // (exactly n bytes, 16-byte aligned)
	memcpy(in, data, n);
	std::vector<inf::HostMember> chain;
	size_t total = 0;
	if (!inf::walk_members(in, n, &chain, &total)) { free(in); return 100; }
	text.assign(total, '\0');
	inf::Tables *T = new inf::Tables;
	uint32_t status = 0;
	size_t out_off = 0;
	for (size_t m = 0; m < chain.size() && !status; ++m) {
		const inf::HostMember &h = chain[m];
		uint8_t *stage = (uint8_t *) malloc(h.isize ? h.isize : 1);
		uint32_t produced = 0;
		uint32_t st = inf::inflate_member(in, (uint32_t) (h.at + h.payload), (uint32_t) (h.at + h.size - 8), stage, h.isize, *T, &produced);
		if (st == inf::kOk) {
			uint32_t crc = 0;
			for (int tid = 0; tid < inf::kNT; ++tid) crc ^= inf::crc_part(stage, h.isize, tid, inf::kNT, tab.data(), tab.data() + 256);
			if (crc != inf::load_le32(in + h.at + h.size - 8)) st = inf::kCrcMismatch;
			else for (int tid = 0; tid < inf::kNT; ++tid) inf::copy_out(stage, h.isize, (uint8_t *) &text[0] + out_off, tid, inf::kNT);
		}
		free(stage);
		if (st != inf::kOk) { status = st; *bad_member = (long long) m; }
		out_off += h.isize;
	}
	delete T;
	free(in);
	return status;
}

static int cmd_records(const char *path, const char *out_path) {
	std::vector<char> file;
	if (!read_file(path, file)) return 2;
	// (a heap block of exactly the file's size)
	char *p = (char *) malloc(file.size() ? file.size() : 1);
	memcpy(p, file.data(), file.size());
	const size_t n = file.size();
	const bi::Format fmt = bi::detect(p, n, true);
	std::string out, err;
	auto put = [&](const bi::View &v) {
		out.append(v.name, v.name_len); out.push_back('\t'); out.append(v.seq, v.seq_len); out.push_back('\t');
		if (v.qual_len) out.append(v.qual, v.qual_len); else out.push_back('*');
		out.push_back('\n');
	};
	bool ok = true;
	if (fmt == bi::kBam) {
		ok = bi::bam_walk((const uint8_t *) p, n, [&](size_t at, size_t, uint32_t ls) {
			char *store = (char *) malloc(bi::bam_store_bytes(ls) + 1);   // (exactly what the decoder may use, + 1 so that it is never 0)
			bi::View v;
			bi::bam_decode((const uint8_t *) p, at, v, store);
			put(v);
			free(store);
		}, &err);
	} else if (fmt == bi::kSam) {
		for (size_t at = 0, next = 0; ok && at < n; at = next) {
			if (!bi::sam_is_record(p, n, at, &next)) continue;
			std::vector<char> store(bi::sam_store_bytes(at, next) + 1);
			bi::View v;
			if (!bi::sam_decode(p, at, next, v, store.data())) { err = "SAM input: sequence and quality lengths differ (" + std::string(v.name, v.name_len) + ")"; ok = false; break; }
			put(v);
		}
	} else {
		err = "neither SAM nor BAM"; ok = false;
	}
	free(p);
	if (!ok) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
	FILE *f = fopen(out_path, "wb");
	if (!f) return 2;
	fwrite(out.data(), 1, out.size(), f);
	fclose(f);
	return 0;
}

int main(int argc, char **argv) {
	if (argc < 3) return 2;
	const std::string cmd = argv[1];
	if (cmd == "detect") {
		const bi::Format f = bi::detect_file(argv[2]);
		printf("%s\n", f == bi::kBam ? "bam" : f == bi::kSam ? "sam" : "fastx");
		return 0;
	}
	if (cmd == "inflate" && argc >= 4) {
		std::vector<char> z;
		if (!read_file(argv[2], z)) return 2;
		std::string text;
		long long bad = -1;
		const uint32_t st = inflate_run(z.data(), z.size(), text, &bad);
		if (st) { printf("member %lld status %u\n", bad, st); return 3; }
		FILE *f = fopen(argv[3], "wb");
		if (!f) return 2;
		fwrite(text.data(), 1, text.size(), f);
		fclose(f);
		return 0;
	}
	if (cmd == "cases" && argc >= 4) {
		std::vector<char> all;
		if (!read_file(argv[2], all)) return 2;
		FILE *f = fopen(argv[3], "wb");
		if (!f) return 2;
		for (size_t at = 0; at + 4 <= all.size();) {
			uint32_t n;
			memcpy(&n, all.data() + at, 4);
			at += 4;
			if (n > all.size() - at) return 2;
			std::string text;
			long long bad = -1;
			uint32_t st = inflate_run(all.data() + at, n, text, &bad);
			at += n;
			if (st) text.clear();
			const uint32_t tn = (uint32_t) text.size();
			fwrite(&st, 4, 1, f); fwrite(&tn, 4, 1, f); fwrite(text.data(), 1, tn, f);
		}
		fclose(f);
		return 0;
	}
	if (cmd == "records" && argc >= 4) return cmd_records(argv[2], argv[3]);
	if (cmd == "index" && argc >= 4) {
		std::vector<char> file;
		if (!read_file(argv[2], file)) return 2;
		const uint8_t *p = (const uint8_t *) file.data();
		std::string err;
		size_t k = 0;
		const size_t step = (size_t) atoi(argv[3]);
		if (!bi::bam_walk(p, file.size(), [&](size_t at, size_t, uint32_t) { if (k++ % step == 0) printf("%zu\n", at); }, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
		printf("%zu\n", k);
		return 0;
	}
	return 2;
}
