// bam_sort.cpp -- host side of `ngm-hip --sort` (include/ngm_pipeline.h, ngm_bam_sort_*): the records of a whole run stay in HBM in segments,
// one stable radix sort over their coordinate keys, a byte-granular gather of the sorted stream chunk by chunk into the BGZF compressor,
// and the arrays of the BAI file.  Kernels: csrc/bam_sort_device.h; the host-only parts (walk, key, serialiser): csrc/bam_sort.h.
// With ngm_bam_sort_set_markdup: duplicates get flag 0x400 in the segments before the sort reads them (mark_duplicates below; the rules
// and the keys: csrc/markdup.h, the kernels: csrc/markdup_device.h).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>   // (after <cstring>: its texture iterator calls the host's memset)

#include "../../include/ngm_pipeline.h"
#include "bam_sort_device.h"
#include "device_util.h"
#include "markdup_device.h"
#include "refindex.h"

namespace bs = ngm::bamsort;
namespace md = ngm::markdup;

using ngm::Buf;
using ngm::DeviceGuard;
using ngm::blocks_of;

namespace {
struct Segment {
	uint64_t seq = 0;
	Buf<uint8_t> d;                // the run's bytes, 16 bytes of padding behind them
	size_t bytes = 0;
	Buf<uint32_t> d_rec_off;       // where its records start
	uint32_t n_rec = 0;
};

}  // namespace

struct ngm_bam_sort {
	int device = 0;
	size_t chunk_bytes = 0, max_bytes = 0;
	std::mutex mu;
	hipStream_t st = nullptr, st_gather = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, evg[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
	int grid = 256;
	std::vector<Segment> segs;
	std::unordered_set<uint64_t> seqs;
	uint64_t total_bytes = 0, n_rec = 0;
	bool finished = false, sorted = false;
	int n_ref = 0;
	// after finish: the sorted order
	Buf<uint64_t> key, u, s_ptr;
	Buf<uint32_t> s_end, s_bin_flag;
	uint64_t n_no_coor = 0;
	// the stream
	Buf<uint8_t> chunk[2];
	long long gathered[2] = {-1, -1};   // which chunk of the stream a buffer holds (its gather may still run: evg[b][1])
	long long timed[2] = {-1, -1};      // ... and the chunk whose gather time ms[2] already holds
	// scratch of add (under mu): counts and bases per range, the first bad range, the scan's storage, the host route's range offsets
	Buf<uint32_t> w_count, w_base, w_bad, w_off;
	Buf<uint8_t> w_tmp;
	ngm_bgzf *bz = nullptr;
	uint64_t next_chunk = 0, n_chunks = 0;
	std::vector<uint64_t> C;            // compressed bytes in front of member k
	// statistics
	uint64_t n_bins = 0;
	float ms[5] = {0, 0, 0, 0, 0};
	std::string bai;
	uint64_t bai_first = ~0ull;
	// --markdup (ngm_bam_sort_set_markdup): the six counts and the kernel ms of marking / its sorts
	bool markdup = false;
	uint64_t md_counts[md::kCounters] = {0, 0, 0, 0, 0, 0};
	float md_ms[2] = {0, 0};
};

extern "C" ngm_bam_sort *ngm_bam_sort_create(const ngm_bam_sort_params *p) {
	if (!p) { ngm::pipeline_set_error("ngm_bam_sort_create: bad arguments"); return nullptr; }
	if (hipSetDevice(p->device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", p->device); return nullptr; }
	ngm_bam_sort *s = new ngm_bam_sort();
	s->device = p->device;
	const size_t want = p->chunk_bytes ? p->chunk_bytes : (size_t) 512 * bs::kMember;   // default: 512 members, 31.9 MiB
	s->chunk_bytes = std::max<size_t>(want / bs::kMember, 1) * bs::kMember;
	s->max_bytes = p->max_bytes;
	hipDeviceProp_t prop;
	bool ok = hipGetDeviceProperties(&prop, p->device) == hipSuccess;
	if (ok) s->grid = prop.multiProcessorCount;
	ok = ok && hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&s->st_gather, hipStreamNonBlocking) == hipSuccess;
	ok = ok && hipEventCreate(&s->ev0) == hipSuccess && hipEventCreate(&s->ev1) == hipSuccess;
	for (int b = 0; b < 2; ++b) for (int e = 0; e < 2; ++e) ok = ok && hipEventCreate(&s->evg[b][e]) == hipSuccess;
	if (ok) { s->bz = ngm_bgzf_create(p->device); if (!s->bz) { ngm_bam_sort_destroy(s); return nullptr; } }
	if (!ok) { ngm::pipeline_set_error("ngm_bam_sort_create: set-up failed on device %d (%s)", p->device, hipGetErrorString(hipGetLastError())); ngm_bam_sort_destroy(s); return nullptr; }
	return s;
}

extern "C" void ngm_bam_sort_destroy(ngm_bam_sort *s) {
	if (!s) return;
	DeviceGuard g(s->device);
	if (s->st) (void) hipStreamSynchronize(s->st);
	if (s->st_gather) (void) hipStreamSynchronize(s->st_gather);
	ngm_bgzf_destroy(s->bz);
	if (s->ev0) (void) hipEventDestroy(s->ev0);
	if (s->ev1) (void) hipEventDestroy(s->ev1);
	for (int b = 0; b < 2; ++b) for (int e = 0; e < 2; ++e) if (s->evg[b][e]) (void) hipEventDestroy(s->evg[b][e]);
	if (s->st) (void) hipStreamDestroy(s->st);
	if (s->st_gather) (void) hipStreamDestroy(s->st_gather);
	delete s;
}

namespace {
int out_of_memory(const ngm_bam_sort *s, const char *what, size_t bytes) {
	ngm::pipeline_set_error("out of device memory for %s (%zu bytes; the sorter holds %.3f GiB of records)", what, bytes, (double) s->total_bytes / (double) (1ull << 30));
	return -12;
}

// d_off: n_ranges + 1 offsets into the segment's bytes, on the device.  Record offsets from them; the records are checked on the way.
// expect_records >= 0 (the host has walked the chain): count, scan and write in one go, one synchronisation; < 0 (the device formatter's
// units): the count comes back first, for the size of the offsets.  The scratch arrays are the sorter's: no allocation but the segment's own.
int index_segment(ngm_bam_sort *s, Segment &sg, const uint32_t *d_off, uint32_t n_ranges, long long expect_records) {
	size_t tb = 0;
	NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, (uint32_t *) nullptr, (uint32_t *) nullptr, 0u, (size_t) n_ranges + 1, rocprim::plus<uint32_t>(), s->st));
	if (s->w_count.grow((size_t) n_ranges + 1) || s->w_base.grow((size_t) n_ranges + 1) || s->w_bad.grow(1) || s->w_tmp.grow(tb + 16)) return out_of_memory(s, "record offsets", ((size_t) n_ranges + 1) * 8 + tb);
	auto write = [&](uint32_t cap) -> int {
		if (cap == 0) return 0;
		if (sg.d_rec_off.alloc(cap)) return out_of_memory(s, "record offsets", (size_t) cap * 4);
		hipLaunchKernelGGL(bs::walk_ranges_kernel<true>, dim3(blocks_of(n_ranges)), dim3(256), 0, s->st, (const uint8_t *) sg.d.p, d_off, n_ranges, (uint32_t *) nullptr, (const uint32_t *) s->w_base.p,
				sg.d_rec_off.p, cap, s->w_bad.p);
		NGM_HIP_TRY(hipGetLastError());
		return 0;
	};
	NGM_HIP_TRY(hipMemsetAsync(s->w_bad.p, 0xFF, 4, s->st));
	NGM_HIP_TRY(hipMemsetAsync(s->w_count.p + n_ranges, 0, 4, s->st));
	hipLaunchKernelGGL(bs::walk_ranges_kernel<false>, dim3(blocks_of(n_ranges)), dim3(256), 0, s->st, (const uint8_t *) sg.d.p, d_off, n_ranges, s->w_count.p, (const uint32_t *) nullptr,
			(uint32_t *) nullptr, 0u, s->w_bad.p);
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(rocprim::exclusive_scan(s->w_tmp.p, tb, s->w_count.p, s->w_base.p, 0u, (size_t) n_ranges + 1, rocprim::plus<uint32_t>(), s->st));
	if (expect_records >= 0) { if (int rc = write((uint32_t) expect_records)) return rc; }
	uint32_t h_bad = 0, h_total = 0;
	NGM_HIP_TRY(hipMemcpyAsync(&h_bad, s->w_bad.p, 4, hipMemcpyDeviceToHost, s->st));
	NGM_HIP_TRY(hipMemcpyAsync(&h_total, s->w_base.p + n_ranges, 4, hipMemcpyDeviceToHost, s->st));
	NGM_HIP_TRY(hipStreamSynchronize(s->st));
	if (h_bad != 0xFFFFFFFFu || (expect_records >= 0 && (long long) h_total != expect_records)) {
		ngm::pipeline_set_error("ngm_bam_sort_add: seq %llu: the records of range %u do not form a chain of block_size that ends with it", (unsigned long long) sg.seq, h_bad);
		return -22;
	}
	sg.n_rec = h_total;
	if (expect_records < 0) {
		if (int rc = write(h_total)) return rc;
		NGM_HIP_TRY(hipStreamSynchronize(s->st));   // (d_off is the mapper's: it is free again when this returns)
	}
	return 0;
}

// the common part of the two add routes, under the lock: refusals, the segment, its record offsets
int add_segment(ngm_bam_sort *s, uint64_t seq, const void *src, bool src_on_device, size_t n_bytes, const uint32_t *h_off, const uint32_t *d_off, uint32_t n_ranges, long long expect_records) {
	if (s->finished) { ngm::pipeline_set_error("ngm_bam_sort_add: seq %llu: add after ngm_bam_sort_finish", (unsigned long long) seq); return -22; }
	if (s->seqs.count(seq)) { ngm::pipeline_set_error("ngm_bam_sort_add: seq %llu was added before (duplicate seq)", (unsigned long long) seq); return -22; }
	if (s->max_bytes && s->total_bytes + n_bytes > s->max_bytes) {
		ngm::pipeline_set_error("ngm_bam_sort_add: seq %llu: %llu bytes of records exceed max_bytes %zu", (unsigned long long) seq, (unsigned long long) (s->total_bytes + n_bytes), s->max_bytes);
		return -12;
	}
	s->seqs.insert(seq);
	if (n_bytes == 0) return 0;
	DeviceGuard g(s->device);
	Segment sg;
	sg.seq = seq; sg.bytes = n_bytes;
	if (sg.d.alloc(n_bytes + 16)) { s->seqs.erase(seq); return out_of_memory(s, "a segment of records", n_bytes + 16); }
	int rc = 0;
	auto body = [&]() -> int {
		NGM_HIP_TRY(hipMemsetAsync(sg.d.p + n_bytes, 0, 16, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(sg.d.p, src, n_bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
		if (h_off) {
			if (s->w_off.grow((size_t) n_ranges + 1)) return out_of_memory(s, "range offsets", ((size_t) n_ranges + 1) * 4);
			NGM_HIP_TRY(hipMemcpyAsync(s->w_off.p, h_off, ((size_t) n_ranges + 1) * 4, hipMemcpyHostToDevice, s->st));   // (pageable memory: staged before the call returns)
		}
		return index_segment(s, sg, h_off ? s->w_off.p : d_off, n_ranges, expect_records);
	};
	rc = body();
	if (rc < 0) { (void) hipStreamSynchronize(s->st); s->seqs.erase(seq); return rc; }   // (the segment goes behind the synchronisation)
	s->total_bytes += n_bytes;
	s->n_rec += sg.n_rec;
	s->segs.push_back(std::move(sg));
	return 0;
}
}  // namespace

extern "C" int ngm_bam_sort_add(ngm_bam_sort *s, uint64_t seq, const void *records, size_t n_bytes) {
	if (!s || (!records && n_bytes)) { ngm::pipeline_set_error("ngm_bam_sort_add: bad arguments"); return -22; }
	// the walk needs no lock: it validates the caller's bytes before anything of them reaches the device
	std::vector<uint32_t> notes;
	uint64_t n_records = 0;
	std::string err;
	if (!bs::walk((const uint8_t *) records, n_bytes, &notes, &n_records, &err)) { ngm::pipeline_set_error("ngm_bam_sort_add: seq %llu: %s", (unsigned long long) seq, err.c_str()); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	return add_segment(s, seq, records, false, n_bytes, notes.data(), nullptr, (uint32_t) (notes.size() - 1), (long long) n_records);
}

// the device formatter's hand-over: d_records / d_unit_off (units + 1 offsets, the last one n_bytes) are in the sorter's device memory and complete
int ngm::bam_sort_add_device(ngm_bam_sort *s, uint64_t seq, const void *d_records, size_t n_bytes, const uint32_t *d_unit_off, size_t units) {
	if (!s || (!d_records && n_bytes) || !d_unit_off || units > 0x7fffffffu || n_bytes > bs::kMaxRun) { ngm::pipeline_set_error("ngm_bam_sort_add (device): bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	return add_segment(s, seq, d_records, true, n_bytes, nullptr, d_unit_off, (uint32_t) units, -1);
}
int ngm::bam_sort_device(const ngm_bam_sort *s) { return s ? s->device : -1; }

extern "C" int ngm_bam_sort_set_markdup(ngm_bam_sort *s, int on) {
	if (!s) { ngm::pipeline_set_error("ngm_bam_sort_set_markdup: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	if (s->finished || !s->seqs.empty()) { ngm::pipeline_set_error("ngm_bam_sort_set_markdup: duplicate marking is chosen before the first ngm_bam_sort_add"); return -22; }
	s->markdup = on != 0;
	return 0;
}

namespace {
// --markdup: flag 0x400 into the records of the segments (sorted by seq), by the rules of csrc/markdup.h.  Runs before the sort's own arrays
// exist and frees its scratch before it returns -- at most 48 bytes per record (the pair round) against the sort's 56 and more.
// Ends: one kernel over the run order.  Pairs: the pair keys in slots of two records, a stable radix sort by the high half and one by the
// low half (the 128-bit order), group heads, scores where a group has more than one pair, arg-best by atomicMax on the group head's entry,
// marks.  Fragments: the same over one sort of all end keys; a group that holds an end of a pair marks its fragments without a score.
int mark_duplicates(ngm_bam_sort *s) {
	const uint64_t n = s->n_rec, m = (n + 1) / 2;
	hipStream_t st = s->st;
	auto timed = [&](int which, auto &&work) -> int {   // kernel ms by events, as for the sort itself
		NGM_HIP_TRY(hipEventRecord(s->ev0, st));
		if (int rc = work()) return rc;
		NGM_HIP_TRY(hipEventRecord(s->ev1, st));
		NGM_HIP_TRY(hipStreamSynchronize(st));
		float t = 0.f;
		if (hipEventElapsedTime(&t, s->ev0, s->ev1) == hipSuccess) s->md_ms[which] += t;
		return 0;
	};
	Buf<uint8_t> tmp;
	auto sort64 = [&](auto keys_in, uint64_t *keys_out, auto vals_in, uint32_t *vals_out, uint64_t count) -> int {
		size_t tb = 0;
		NGM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys_in, keys_out, vals_in, vals_out, (size_t) count, 0, 64, st));
		if (tb + 16 > tmp.cap && tmp.alloc(tb + 16)) return out_of_memory(s, "the sort of duplicate marking", tb);
		return timed(1, [&]() -> int { NGM_HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, keys_in, keys_out, vals_in, vals_out, (size_t) count, 0, 64, st)); return 0; });
	};
	auto head_places = [&](uint32_t *hp, uint64_t count) -> int {   // in place: hp[r] = the place of r's group head
		size_t tb = 0;
		NGM_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, hp, hp, (size_t) count, rocprim::maximum<uint32_t>(), st));
		if (tb + 16 > tmp.cap && tmp.alloc(tb + 16)) return out_of_memory(s, "a scan of duplicate marking", tb);
		NGM_HIP_TRY(rocprim::inclusive_scan(tmp.p, tb, hp, hp, (size_t) count, rocprim::maximum<uint32_t>(), st));
		return 0;
	};
	const rocprim::counting_iterator<uint32_t> iota(0u);
	Buf<uint64_t> ptr, ek;
	Buf<uint8_t> kind, need;
	Buf<uint32_t> score;
	Buf<unsigned long long> ctr;
	if (ptr.alloc(n) || ek.alloc(n) || kind.alloc(n) || need.alloc(n) || score.alloc(n) || ctr.alloc(md::kCounters)) return out_of_memory(s, "duplicate marking", (size_t) n * 22);
	unsigned long long h_ctr[md::kCounters] = {0, 0, 0, 0, 0, 0};
	if (int rc = timed(0, [&]() -> int {
		NGM_HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(h_ctr), st));
		uint64_t g0 = 0;
		for (const Segment &sg : s->segs) {
			if (!sg.n_rec) continue;
			hipLaunchKernelGGL(md::ptrs_kernel, dim3(blocks_of(sg.n_rec)), dim3(256), 0, st, (const uint8_t *) sg.d.p, (const uint32_t *) sg.d_rec_off.p, sg.n_rec, g0, ptr.p);
			NGM_HIP_TRY(hipGetLastError());
			g0 += sg.n_rec;
		}
		hipLaunchKernelGGL(md::ends_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const uint64_t *) ptr.p, n, ek.p, kind.p, ctr.p);
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
		return 0;
	})) return rc;
	const uint64_t n_exam = h_ctr[md::kExamined], n_pairs = h_ctr[md::kPairs];
	if (n_pairs > 0) {
		Buf<uint64_t> hi, lo, k1, k2;
		Buf<uint32_t> i1, i2;
		if (hi.alloc(m) || lo.alloc(m) || k1.alloc(m) || k2.alloc(m) || i1.alloc(m) || i2.alloc(m)) return out_of_memory(s, "the pairs of duplicate marking", (size_t) m * 40);
		if (int rc = timed(0, [&]() -> int {
			NGM_HIP_TRY(hipMemsetAsync(hi.p, 0xFF, m * 8, st));
			NGM_HIP_TRY(hipMemsetAsync(lo.p, 0xFF, m * 8, st));
			NGM_HIP_TRY(hipMemsetAsync(need.p, 0, n, st));
			hipLaunchKernelGGL(md::pair_keys_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const uint64_t *) ek.p, (const uint8_t *) kind.p, n, lo.p, hi.p);
			NGM_HIP_TRY(hipGetLastError());
			return 0;
		})) return rc;
		// stable, the high half first: (lo, hi) ascending, equal keys in run order; the slots without a pair (kNoKey) end up behind the n_pairs pairs
		if (int rc = sort64((const uint64_t *) hi.p, k1.p, iota, i1.p, m)) return rc;
		if (int rc = timed(0, [&]() -> int {
			hipLaunchKernelGGL(md::gather64_kernel, dim3(blocks_of(m)), dim3(256), 0, st, (const uint32_t *) i1.p, m, (const uint64_t *) lo.p, k2.p);
			NGM_HIP_TRY(hipGetLastError());
			return 0;
		})) return rc;
		if (int rc = sort64((const uint64_t *) k2.p, k1.p, (const uint32_t *) i1.p, i2.p, m)) return rc;
		// k1: the low halves in their final order, k2: the high halves to match; lo becomes the groups' best, i1 their head places
		unsigned long long *best = (unsigned long long *) lo.p;
		uint32_t *hp = i1.p;
		const dim3 grid(blocks_of(n_pairs));
		if (int rc = timed(0, [&]() -> int {
			hipLaunchKernelGGL(md::gather64_kernel, grid, dim3(256), 0, st, (const uint32_t *) i2.p, n_pairs, (const uint64_t *) hi.p, k2.p);
			NGM_HIP_TRY(hipGetLastError());
			NGM_HIP_TRY(hipMemsetAsync(best, 0, n_pairs * 8, st));
			hipLaunchKernelGGL(md::heads_kernel, grid, dim3(256), 0, st, (const uint64_t *) k1.p, (const uint64_t *) k2.p, n_pairs, hp);
			NGM_HIP_TRY(hipGetLastError());
			if (int rc = head_places(hp, n_pairs)) return rc;
			hipLaunchKernelGGL(md::pair_need_kernel, grid, dim3(256), 0, st, (const uint32_t *) i2.p, (const uint32_t *) hp, n_pairs, (const uint8_t *) kind.p, need.p);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::scores_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const uint64_t *) ptr.p, n, (const uint8_t *) need.p, score.p);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::pair_best_kernel, grid, dim3(256), 0, st, (const uint32_t *) i2.p, (const uint32_t *) hp, n_pairs, (const uint8_t *) kind.p, (const uint32_t *) score.p, best);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::pair_mark_kernel, grid, dim3(256), 0, st, (const uint32_t *) i2.p, (const uint32_t *) hp, n_pairs, (const uint8_t *) kind.p, (const uint32_t *) score.p,
					(const unsigned long long *) best, (const uint64_t *) ptr.p, ctr.p);
			NGM_HIP_TRY(hipGetLastError());
			return 0;
		})) return rc;
	}
	if (n_exam > 0) {
		Buf<uint64_t> ek_s;
		Buf<uint32_t> idx, hp;
		if (ek_s.alloc(n) || idx.alloc(n)) return out_of_memory(s, "the end keys of duplicate marking", (size_t) n * 12);
		if (int rc = sort64((const uint64_t *) ek.p, ek_s.p, iota, idx.p, n)) return rc;   // (the ignored records, kNoKey, behind the n_exam examined ones)
		tmp.release();
		if (hp.alloc(n_exam)) return out_of_memory(s, "the groups of duplicate marking", (size_t) n_exam * 4);
		unsigned long long *best = (unsigned long long *) ek.p;   // (the unsorted keys are done with)
		const dim3 grid(blocks_of(n_exam));
		if (int rc = timed(0, [&]() -> int {
			NGM_HIP_TRY(hipMemsetAsync(best, 0, n_exam * 8, st));
			NGM_HIP_TRY(hipMemsetAsync(need.p, 0, n, st));
			hipLaunchKernelGGL(md::heads_kernel, grid, dim3(256), 0, st, (const uint64_t *) ek_s.p, (const uint64_t *) nullptr, n_exam, hp.p);
			NGM_HIP_TRY(hipGetLastError());
			if (int rc = head_places(hp.p, n_exam)) return rc;
			if (n_pairs > 0) {
				hipLaunchKernelGGL(md::pair_ends_kernel, grid, dim3(256), 0, st, (const uint32_t *) idx.p, (const uint32_t *) hp.p, n_exam, (const uint8_t *) kind.p, best);
				NGM_HIP_TRY(hipGetLastError());
			}
			hipLaunchKernelGGL(md::frag_need_kernel, grid, dim3(256), 0, st, (const uint32_t *) idx.p, (const uint32_t *) hp.p, n_exam, (const uint8_t *) kind.p, (const unsigned long long *) best, need.p);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::scores_kernel, dim3(blocks_of(n)), dim3(256), 0, st, (const uint64_t *) ptr.p, n, (const uint8_t *) need.p, score.p);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::frag_best_kernel, grid, dim3(256), 0, st, (const uint32_t *) idx.p, (const uint32_t *) hp.p, n_exam, (const uint8_t *) kind.p, (const uint32_t *) score.p, best);
			NGM_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(md::frag_mark_kernel, grid, dim3(256), 0, st, (const uint32_t *) idx.p, (const uint32_t *) hp.p, n_exam, (const uint8_t *) kind.p, (const uint32_t *) score.p,
					(const unsigned long long *) best, (const uint64_t *) ptr.p, ctr.p);
			NGM_HIP_TRY(hipGetLastError());
			return 0;
		})) return rc;
	}
	NGM_HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, sizeof(h_ctr), hipMemcpyDeviceToHost, st));
	NGM_HIP_TRY(hipStreamSynchronize(st));
	for (int k = 0; k < md::kCounters; ++k) s->md_counts[k] = h_ctr[k];
	return 0;
}
}  // namespace

extern "C" int ngm_bam_sort_finish(ngm_bam_sort *s, int n_ref) {
	if (!s || n_ref < 0) { ngm::pipeline_set_error("ngm_bam_sort_finish: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	if (s->finished) { ngm::pipeline_set_error("ngm_bam_sort_finish: called twice"); return -22; }
	s->finished = true;
	s->n_ref = n_ref;
	DeviceGuard g(s->device);
	std::sort(s->segs.begin(), s->segs.end(), [](const Segment &a, const Segment &b) { return a.seq < b.seq; });
	const uint64_t n = s->n_rec;
	if (n >= 0xFFFFFFFFull) { ngm::pipeline_set_error("ngm_bam_sort_finish: %llu records, more than the 32-bit record numbers of the sort hold", (unsigned long long) n); return -22; }
	s->n_chunks = (s->total_bytes + s->chunk_bytes - 1) / s->chunk_bytes;
	s->C.assign(1, 0);
	if (n == 0) { s->sorted = true; return 0; }
	if (s->markdup) { if (int rc = mark_duplicates(s)) return rc; }   // (its scratch is free again before the sort's arrays are allocated)
	Buf<uint64_t> key_in, ptr, s_len;
	Buf<uint32_t> idx_in, idx, len, end_in, bin_flag;
	Buf<unsigned long long> ctr;   // [0] the first record to refuse, [1] records without a reference
	if (key_in.alloc(n) || s->key.alloc(n) || ptr.alloc(n) || idx_in.alloc(n) || idx.alloc(n) || len.alloc(n) || end_in.alloc(n) || bin_flag.alloc(n) || ctr.alloc(2))
		return out_of_memory(s, "the sort's arrays", (size_t) n * 44);
	const unsigned long long ctr0[2] = {~0ull, 0ull};
	NGM_HIP_TRY(hipMemcpyAsync(ctr.p, ctr0, 16, hipMemcpyHostToDevice, s->st));
	NGM_HIP_TRY(hipEventRecord(s->ev0, s->st));
	uint64_t g0 = 0;
	for (const Segment &sg : s->segs) {
		if (!sg.n_rec) continue;
		hipLaunchKernelGGL(bs::keys_kernel, dim3(blocks_of(sg.n_rec)), dim3(256), 0, s->st, (const uint8_t *) sg.d.p, (const uint32_t *) sg.d_rec_off.p, sg.n_rec, g0, n_ref, key_in.p, idx_in.p, ptr.p,
				len.p, end_in.p, bin_flag.p, ctr.p, ctr.p + 1);
		NGM_HIP_TRY(hipGetLastError());
		g0 += sg.n_rec;
	}
	NGM_HIP_TRY(hipEventRecord(s->ev1, s->st));
	unsigned long long h_ctr[2] = {0, 0};
	NGM_HIP_TRY(hipMemcpyAsync(h_ctr, ctr.p, 16, hipMemcpyDeviceToHost, s->st));
	NGM_HIP_TRY(hipStreamSynchronize(s->st));
	(void) hipEventElapsedTime(&s->ms[0], s->ev0, s->ev1);
	if (h_ctr[0] != ~0ull) {
		uint64_t g = h_ctr[0] >> 8, seq = 0, at = g;
		for (const Segment &sg : s->segs) { if (at < sg.n_rec) { seq = sg.seq; break; } at -= sg.n_rec; }
		const int why = (int) (h_ctr[0] & 0xFF);
		ngm::pipeline_set_error("ngm_bam_sort_finish: seq %llu, record %llu: %s", (unsigned long long) seq, (unsigned long long) at,
				why == bs::kBadRef ? "its refID is not below n_ref (or below -1)" : why == bs::kBadPos ? "it has a reference and a negative position" :
				"it ends above 2^29, beyond what a BAI index reaches");
		return -22;
	}
	s->n_no_coor = h_ctr[1];
	// one stable radix sort of (key, record number): equal keys keep the run order
	size_t tb = 0;
	NGM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, key_in.p, s->key.p, idx_in.p, idx.p, (size_t) n, 0, 64, s->st));
	{
		Buf<uint8_t> tmp;
		if (tmp.alloc(tb + 16)) return out_of_memory(s, "the sort", tb);
		NGM_HIP_TRY(hipEventRecord(s->ev0, s->st));
		NGM_HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, key_in.p, s->key.p, idx_in.p, idx.p, (size_t) n, 0, 64, s->st));
		NGM_HIP_TRY(hipEventRecord(s->ev1, s->st));
		NGM_HIP_TRY(hipStreamSynchronize(s->st));
		(void) hipEventElapsedTime(&s->ms[1], s->ev0, s->ev1);
	}
	key_in.release(); idx_in.release();
	if (s_len.alloc(n + 1) || s->u.alloc(n + 1) || s->s_ptr.alloc(n) || s->s_end.alloc(n) || s->s_bin_flag.alloc(n)) return out_of_memory(s, "the sorted arrays", (size_t) n * 32);
	NGM_HIP_TRY(hipMemsetAsync(s_len.p + n, 0, 8, s->st));
	hipLaunchKernelGGL(bs::permute_kernel, dim3(blocks_of(n)), dim3(256), 0, s->st, (const uint32_t *) idx.p, n, (const uint64_t *) ptr.p, (const uint32_t *) len.p, (const uint32_t *) end_in.p,
			(const uint32_t *) bin_flag.p, s->s_ptr.p, s_len.p, s->s_end.p, s->s_bin_flag.p);
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, s_len.p, s->u.p, (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s->st));
	{
		Buf<uint8_t> tmp;
		if (tmp.alloc(tb + 16)) return out_of_memory(s, "a scan", tb);
		NGM_HIP_TRY(rocprim::exclusive_scan(tmp.p, tb, s_len.p, s->u.p, (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s->st));
		uint64_t total = 0;
		NGM_HIP_TRY(hipMemcpyAsync(&total, s->u.p + n, 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipStreamSynchronize(s->st));
		if (total != s->total_bytes) { ngm::pipeline_set_error("ngm_bam_sort_finish: the records' lengths sum to %llu bytes, %llu were added", (unsigned long long) total, (unsigned long long) s->total_bytes); return -5; }
	}
	s->sorted = true;
	return 0;
}

namespace {
// the gather of chunk c into buffer c & 1, on the gather stream
int launch_gather(ngm_bam_sort *s, uint64_t c) {
	const int b = (int) (c & 1);
	const uint64_t s0 = c * s->chunk_bytes, nb = std::min<uint64_t>(s->chunk_bytes, s->total_bytes - s0);
	if (!s->chunk[b].p && s->chunk[b].alloc(std::min<uint64_t>(s->chunk_bytes, s->total_bytes) + 16)) return out_of_memory(s, "a chunk of the sorted stream", s->chunk_bytes);
	NGM_HIP_TRY(hipEventRecord(s->evg[b][0], s->st_gather));
	const unsigned grid = (unsigned) std::min<uint64_t>((nb + bs::kGatherBlockBytes - 1) / bs::kGatherBlockBytes, (uint64_t) s->grid * 8);
	hipLaunchKernelGGL(bs::gather_kernel, dim3(grid), dim3(256), 0, s->st_gather, (const uint64_t *) s->u.p, (const uint64_t *) s->s_ptr.p, s->n_rec, s0, nb, s->chunk[b].p);
	NGM_HIP_TRY(hipGetLastError());
	NGM_HIP_TRY(hipEventRecord(s->evg[b][1], s->st_gather));
	s->gathered[b] = (long long) c;
	return 0;
}
}  // namespace

extern "C" long long ngm_bam_sort_next(ngm_bam_sort *s, void *out, size_t out_cap) {
	if (!s) { ngm::pipeline_set_error("ngm_bam_sort_next: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	if (!s->sorted) { ngm::pipeline_set_error("ngm_bam_sort_next: ngm_bam_sort_finish has not succeeded"); return -22; }
	if (s->next_chunk >= s->n_chunks) return 0;
	const uint64_t c = s->next_chunk, s0 = c * s->chunk_bytes, nb = std::min<uint64_t>(s->chunk_bytes, s->total_bytes - s0);
	const size_t need = ngm_bgzf_bound((size_t) nb);
	if (out_cap < need || !out) return (long long) need;
	DeviceGuard g(s->device);
	const int b = (int) (c & 1);
	if (s->gathered[b] != (long long) c) { if (int rc = launch_gather(s, c)) return rc; }
	NGM_HIP_TRY(hipEventSynchronize(s->evg[b][1]));
	float t = 0.f;
	if (s->timed[b] != (long long) c && hipEventElapsedTime(&t, s->evg[b][0], s->evg[b][1]) == hipSuccess) { s->ms[2] += t; s->timed[b] = (long long) c; }   // (once per chunk, also when the call is repeated)
	// the next chunk is gathered (its own stream, the other buffer) while this one is compressed
	if (c + 1 < s->n_chunks) { if (int rc = launch_gather(s, c + 1)) return rc; }
	const long long z = ngm_bgzf_compress_device(s->bz, s->chunk[b].p, (size_t) nb, out, out_cap);
	if (z < 0) return z;
	s->ms[3] += ngm_bgzf_last_kernel_ms(s->bz);
	// the members' sizes: BSIZE of every member just written
	const uint8_t *p = (const uint8_t *) out;
	size_t at = 0, members = 0;
	while (at < (size_t) z) {
		if (at + 18 > (size_t) z) { ngm::pipeline_set_error("ngm_bam_sort_next: the compressor's output is not a run of whole members"); return -5; }
		const size_t size = (size_t) (p[at + 16] | (p[at + 17] << 8)) + 1;
		at += size;
		s->C.push_back(s->C.back() + size);
		++members;
	}
	if (at != (size_t) z || members != (nb + bs::kMember - 1) / bs::kMember) { ngm::pipeline_set_error("ngm_bam_sort_next: %zu members for %llu bytes", members, (unsigned long long) nb); return -5; }
	++s->next_chunk;
	return z;
}

namespace {
int build_index(ngm_bam_sort *s, uint64_t first) {
	const int n_ref = s->n_ref;
	const uint64_t n = s->n_rec, n_coor = n - s->n_no_coor;
	std::vector<uint64_t> h_ref((size_t) n_ref * 4 + 1, 0), h_win_base((size_t) n_ref + 1, 0), h_ioff, h_ckey, h_cbeg, h_cend;
	bs::BaiArrays A;
	A.n_ref = n_ref; A.n_no_coor = s->n_no_coor;
	s->ms[4] = 0.f;
	if (n_coor > 0) {
		Buf<uint64_t> C, vbeg, vend, n_intv, win_base, ref_mapped, ckey, ckey_s, cbeg, cend, cbeg_s, cend_s;
		Buf<uint32_t> head, before, cval, cval_s;
		Buf<unsigned long long> refs, rev, rev_s;   // refs: vbeg, vend, first, last, unmapped, maxend [n_ref each]
		Buf<uint8_t> tmp;
		if (C.alloc(s->C.size()) || vbeg.alloc(n_coor) || vend.alloc(n_coor) || head.alloc(n_coor + 1) || before.alloc(n_coor + 1) || refs.alloc((size_t) n_ref * 6) ||
				n_intv.alloc((size_t) n_ref + 1) || win_base.alloc((size_t) n_ref + 1) || ref_mapped.alloc((size_t) n_ref))
			return out_of_memory(s, "the index arrays", (size_t) n_coor * 24);
		NGM_HIP_TRY(hipMemcpyAsync(C.p, s->C.data(), s->C.size() * 8, hipMemcpyHostToDevice, s->st));
		NGM_HIP_TRY(hipMemsetAsync(refs.p, 0, (size_t) n_ref * 48, s->st));
		bs::IndexArgs I{};
		I.n_coor = n_coor; I.key = s->key.p; I.u = s->u.p; I.s_end = s->s_end.p; I.s_bin_flag = s->s_bin_flag.p; I.C = C.p; I.first = first; I.vbeg = vbeg.p; I.vend = vend.p; I.head = head.p;
		I.ref_vbeg = refs.p; I.ref_vend = refs.p + n_ref; I.ref_first = refs.p + 2 * (size_t) n_ref; I.ref_last = refs.p + 3 * (size_t) n_ref; I.ref_unmapped = refs.p + 4 * (size_t) n_ref;
		I.ref_maxend = refs.p + 5 * (size_t) n_ref;
		NGM_HIP_TRY(hipEventRecord(s->ev0, s->st));
		hipLaunchKernelGGL(bs::index_records_kernel, dim3(blocks_of(n_coor)), dim3(256), 0, s->st, I);
		NGM_HIP_TRY(hipGetLastError());
		size_t tb = 0;
		NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, head.p, before.p, 0u, (size_t) n_coor + 1, rocprim::plus<uint32_t>(), s->st));
		if (tmp.alloc(tb + 16)) return out_of_memory(s, "a scan", tb);
		NGM_HIP_TRY(rocprim::exclusive_scan(tmp.p, tb, head.p, before.p, 0u, (size_t) n_coor + 1, rocprim::plus<uint32_t>(), s->st));
		uint32_t n_chunks = 0;
		NGM_HIP_TRY(hipMemcpyAsync(&n_chunks, before.p + n_coor, 4, hipMemcpyDeviceToHost, s->st));
		// the windows of the references
		hipLaunchKernelGGL(bs::ref_windows_kernel, dim3(blocks_of((uint64_t) n_ref + 1)), dim3(256), 0, s->st, n_ref, (const unsigned long long *) I.ref_maxend, (const unsigned long long *) I.ref_first,
				(const unsigned long long *) I.ref_last, (const unsigned long long *) I.ref_unmapped, n_intv.p, ref_mapped.p);
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, n_intv.p, win_base.p, (uint64_t) 0, (size_t) n_ref + 1, rocprim::plus<uint64_t>(), s->st));
		if (tb + 16 > tmp.cap && tmp.alloc(tb + 16)) return out_of_memory(s, "a scan", tb);
		NGM_HIP_TRY(rocprim::exclusive_scan(tmp.p, tb, n_intv.p, win_base.p, (uint64_t) 0, (size_t) n_ref + 1, rocprim::plus<uint64_t>(), s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_win_base.data(), win_base.p, ((size_t) n_ref + 1) * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipStreamSynchronize(s->st));
		const uint64_t n_win = h_win_base[n_ref];
		// the chunks, stably sorted by (reference, bin)
		if (ckey.alloc(n_chunks) || ckey_s.alloc(n_chunks) || cval.alloc(n_chunks) || cval_s.alloc(n_chunks) || cbeg.alloc(n_chunks) || cend.alloc(n_chunks) || cbeg_s.alloc(n_chunks) ||
				cend_s.alloc(n_chunks) || rev.alloc(n_win) || rev_s.alloc(n_win))
			return out_of_memory(s, "the index arrays", (size_t) n_chunks * 56 + (size_t) n_win * 16);
		hipLaunchKernelGGL(bs::chunks_kernel, dim3(blocks_of(n_coor)), dim3(256), 0, s->st, I, (const uint32_t *) before.p, ckey.p, cval.p, cbeg.p, cend.p);
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, ckey.p, ckey_s.p, cval.p, cval_s.p, (size_t) n_chunks, 0, 64, s->st));
		if (tb + 16 > tmp.cap && tmp.alloc(tb + 16)) return out_of_memory(s, "the sort of the chunks", tb);
		NGM_HIP_TRY(rocprim::radix_sort_pairs(tmp.p, tb, ckey.p, ckey_s.p, cval.p, cval_s.p, (size_t) n_chunks, 0, 64, s->st));
		hipLaunchKernelGGL(bs::chunks_permute_kernel, dim3(blocks_of(n_chunks)), dim3(256), 0, s->st, (const uint32_t *) cval_s.p, (uint64_t) n_chunks, (const uint64_t *) cbeg.p,
				(const uint64_t *) cend.p, cbeg_s.p, cend_s.p);
		NGM_HIP_TRY(hipGetLastError());
		// the linear index
		NGM_HIP_TRY(hipMemsetAsync(rev.p, 0xFF, n_win * 8, s->st));
		hipLaunchKernelGGL(bs::windows_kernel, dim3(blocks_of(n_coor)), dim3(256), 0, s->st, I, (const uint64_t *) win_base.p, n_win, rev.p);
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, rev.p, rev_s.p, (size_t) n_win, rocprim::minimum<unsigned long long>(), s->st));
		if (tb + 16 > tmp.cap && tmp.alloc(tb + 16)) return out_of_memory(s, "a scan", tb);
		NGM_HIP_TRY(rocprim::inclusive_scan(tmp.p, tb, rev.p, rev_s.p, (size_t) n_win, rocprim::minimum<unsigned long long>(), s->st));
		hipLaunchKernelGGL(bs::reverse_kernel, dim3(blocks_of(n_win)), dim3(256), 0, s->st, (const uint64_t *) rev_s.p, n_win, (uint64_t *) rev.p);
		NGM_HIP_TRY(hipGetLastError());
		NGM_HIP_TRY(hipEventRecord(s->ev1, s->st));
		h_ioff.resize(n_win); h_ckey.resize(n_chunks); h_cbeg.resize(n_chunks); h_cend.resize(n_chunks);
		NGM_HIP_TRY(hipMemcpyAsync(h_ioff.data(), rev.p, n_win * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_ckey.data(), ckey_s.p, (size_t) n_chunks * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_cbeg.data(), cbeg_s.p, (size_t) n_chunks * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_cend.data(), cend_s.p, (size_t) n_chunks * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_ref.data(), I.ref_vbeg, (size_t) n_ref * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_ref.data() + n_ref, I.ref_vend, (size_t) n_ref * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_ref.data() + 2 * (size_t) n_ref, ref_mapped.p, (size_t) n_ref * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipMemcpyAsync(h_ref.data() + 3 * (size_t) n_ref, I.ref_unmapped, (size_t) n_ref * 8, hipMemcpyDeviceToHost, s->st));
		NGM_HIP_TRY(hipStreamSynchronize(s->st));
		(void) hipEventElapsedTime(&s->ms[4], s->ev0, s->ev1);
		A.n_chunks = n_chunks;
	}
	A.chunk_key = h_ckey.data(); A.chunk_beg = h_cbeg.data(); A.chunk_end = h_cend.data();
	A.ref_vbeg = h_ref.data(); A.ref_vend = h_ref.data() + n_ref; A.ref_mapped = h_ref.data() + 2 * (size_t) n_ref; A.ref_unmapped = h_ref.data() + 3 * (size_t) n_ref;
	A.win_base = h_win_base.data(); A.ioffset = h_ioff.data();
	bs::bai_serialise(A, s->bai, &s->n_bins);
	s->bai_first = first;
	return 0;
}
}  // namespace

extern "C" long long ngm_bam_sort_index(ngm_bam_sort *s, uint64_t first_member_offset, void *out, size_t out_cap) {
	if (!s) { ngm::pipeline_set_error("ngm_bam_sort_index: bad arguments"); return -22; }
	std::lock_guard<std::mutex> lk(s->mu);
	if (!s->sorted || s->next_chunk < s->n_chunks) { ngm::pipeline_set_error("ngm_bam_sort_index: the virtual offsets are known after the last ngm_bam_sort_next"); return -22; }
	if (s->bai.empty() || s->bai_first != first_member_offset) {
		DeviceGuard g(s->device);
		if (int rc = build_index(s, first_member_offset)) return rc;
	}
	if (!out) return (long long) s->bai.size();
	if (out_cap < s->bai.size()) { ngm::pipeline_set_error("ngm_bam_sort_index: the index has %zu bytes, the buffer %zu", s->bai.size(), out_cap); return -22; }
	memcpy(out, s->bai.data(), s->bai.size());
	return (long long) s->bai.size();
}

extern "C" int ngm_bam_sort_stats(const ngm_bam_sort *s, uint64_t counts[5], float ms[5]) {
	if (!s) return -22;
	if (counts) { counts[0] = s->n_rec; counts[1] = s->total_bytes; counts[2] = s->C.empty() ? 0 : s->C.size() - 1; counts[3] = s->next_chunk; counts[4] = s->n_bins; }
	if (ms) for (int k = 0; k < 5; ++k) ms[k] = s->ms[k];
	return 0;
}

extern "C" int ngm_bam_sort_markdup_stats(const ngm_bam_sort *s, uint64_t counts[6], float ms[2]) {
	if (!s) { ngm::pipeline_set_error("ngm_bam_sort_markdup_stats: bad arguments"); return -22; }
	if (!s->markdup) { ngm::pipeline_set_error("ngm_bam_sort_markdup_stats: duplicate marking is off (ngm_bam_sort_set_markdup)"); return -22; }
	if (!s->sorted) { ngm::pipeline_set_error("ngm_bam_sort_markdup_stats: ngm_bam_sort_finish has not succeeded"); return -22; }
	if (counts) for (int k = 0; k < md::kCounters; ++k) counts[k] = s->md_counts[k];
	if (ms) { ms[0] = s->md_ms[0]; ms[1] = s->md_ms[1]; }
	return 0;
}
