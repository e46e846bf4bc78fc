// bgzf.cpp -- host side of the GPU BGZF compressor (bgzf_device.h) and inflater (bgzf_inflate_device.h): ngm_bgzf_create / _compress /
// _inflate / _destroy (include/ngm_pipeline.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ngm_pipeline.h"
#include "bgzf_device.h"
#include "bgzf_inflate_device.h"
#include "refindex.h"

#define BGZF_HIP_TRY(expr)                                                                      \
	do {                                                                                        \
		hipError_t e_ = (expr);                                                                 \
		if (e_ != hipSuccess) {                                                                 \
			ngm::pipeline_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return -5;                                                                          \
		}                                                                                       \
	} while (0)

using ngm::Buf;
using ngm::PinnedBuf;

struct ngm_bgzf {
	int device = 0;
	hipStream_t st = nullptr;
	// (buffers that grow together are released together before they are allocated anew, and the one allocated last is asked whether they
	// fit: its capacity is 0 after any refusal)
	Buf<uint8_t> d_raw, d_out, d_dense, d_tables;
	Buf<uint32_t> d_sizes;
	Buf<unsigned long long> d_offsets;
	Buf<uint2> d_scratch;
	Buf<unsigned long long> d_phases;
	int grid = 0;
	PinnedBuf<uint32_t> h_sizes;
	PinnedBuf<unsigned long long> h_offsets;
	float last_ms = 0.f;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	// the inflater (set up by the first ngm_bgzf_inflate): two slots, so that one chunk's copies run under its neighbour's kernel
	struct InflateSlot {
		hipStream_t st = nullptr;
		hipEvent_t ev0 = nullptr, ev1 = nullptr;
		Buf<uint8_t> d_in, d_out;
		PinnedBuf<uint8_t> h_in, h_out;
		Buf<ngm::inflate::Member> d_mem;
		PinnedBuf<ngm::inflate::Member> h_mem;
		Buf<uint32_t> d_status;
		PinnedBuf<uint32_t> h_status;
		// the chunk in flight
		size_t first_member = 0, n_members = 0, text_at = 0, text_bytes = 0;
		bool busy = false;
	} inf[2];
	Buf<uint32_t> d_inf_tables;        // CRC byte table [256], x^(8 m) [65537]
	hipEvent_t inf_base = nullptr;     // recorded in front of a call's first kernel: the chunks' kernel intervals are measured from it
	float inf_busy_until = 0.f;        // ms after inf_base up to which the intervals seen so far reach
	bool inf_ready = false;
};

namespace {
constexpr size_t kTabCrc = 0, kTabXpow = 4096, kTabLen = kTabXpow + 4 * (size_t) (ngm::bgzf::kIn + 1), kTabDist = kTabLen + 256, kTabBytes = kTabDist + 512;

uint32_t mulmod(uint32_t a, uint32_t b) {
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b >> 1) ^ ((b & 1u) ? 0xedb88320u : 0u);
	}
	return p;
}
void fill_tables(std::vector<uint8_t> &t) {
	t.assign(kTabBytes, 0);
	uint32_t *crc = (uint32_t *) (t.data() + kTabCrc);
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t c = i;
		for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
		crc[i] = c;
	}
	for (uint32_t i = 0; i < 256; ++i) for (int k = 1; k < 4; ++k) crc[k * 256 + i] = crc[crc[(k - 1) * 256 + i] & 255u] ^ (crc[(k - 1) * 256 + i] >> 8);   // slicing-by-4
	uint32_t *xp = (uint32_t *) (t.data() + kTabXpow);
	xp[0] = 0x80000000u;   // x^0
	for (int m = 1; m <= ngm::bgzf::kIn; ++m) xp[m] = mulmod(xp[m - 1], 0x00800000u);   // * x^8
	static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
	static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
	uint8_t *lc = t.data() + kTabLen, *dc = t.data() + kTabDist;
	for (int l = 3; l <= 258; ++l) { int c = 28; while (lbase[c] > l) --c; lc[l - 3] = (uint8_t) c; }
	auto dcode = [&](int d) { int c = 29; while (dbase[c] > d) --c; return (uint8_t) c; };
	for (int d = 0; d < 256; ++d) dc[d] = dcode(d + 1);
	for (int i = 2; i < 256; ++i) dc[256 + i] = dcode((i << 7) + 1);   // distance - 1 = i * 128 + (0..127): one code for all of them from 257 on
}
}  // namespace

extern "C" ngm_bgzf *ngm_bgzf_create(int device) {
	if (hipSetDevice(device) != hipSuccess) { ngm::pipeline_set_error("hipSetDevice(%d) failed", device); return nullptr; }
	ngm_bgzf *z = new ngm_bgzf();
	z->device = device;
	std::vector<uint8_t> t;
	fill_tables(t);
	hipDeviceProp_t prop;
	bool ok = hipGetDeviceProperties(&prop, device) == hipSuccess;
	z->grid = ok ? prop.multiProcessorCount : 256;
	ok = ok && hipStreamCreateWithFlags(&z->st, hipStreamNonBlocking) == hipSuccess;
	ok = ok && !z->d_tables.alloc(kTabBytes) && hipMemcpy(z->d_tables.p, t.data(), kTabBytes, hipMemcpyHostToDevice) == hipSuccess;
	ok = ok && !z->d_scratch.alloc((size_t) z->grid * ngm::bgzf::kSegs * ngm::bgzf::kMatCap);
	if (getenv("NGM_HIP_CS_PHASES")) ok = ok && !z->d_phases.alloc(8);   // (the diagnostics switch of the search kernels: phases of the deflate kernel too)
	ok = ok && hipEventCreate(&z->ev0) == hipSuccess && hipEventCreate(&z->ev1) == hipSuccess;
	ok = ok && hipFuncSetAttribute((const void *) ngm::bgzf::deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ngm::bgzf::deflate_lds_bytes()) == hipSuccess;
	if (!ok) { ngm::pipeline_set_error("GPU BGZF compressor: set-up failed on device %d (%s)", device, hipGetErrorString(hipGetLastError())); ngm_bgzf_destroy(z); return nullptr; }
	return z;
}

extern "C" void ngm_bgzf_destroy(ngm_bgzf *z) {
	if (!z) return;
	(void) hipSetDevice(z->device);
	if (z->st) (void) hipStreamSynchronize(z->st);
	if (z->ev0) (void) hipEventDestroy(z->ev0);
	if (z->ev1) (void) hipEventDestroy(z->ev1);
	if (z->st) (void) hipStreamDestroy(z->st);
	for (ngm_bgzf::InflateSlot &s : z->inf) {
		if (s.st) (void) hipStreamSynchronize(s.st);
		if (s.ev0) (void) hipEventDestroy(s.ev0);
		if (s.ev1) (void) hipEventDestroy(s.ev1);
		if (s.st) (void) hipStreamDestroy(s.st);
	}
	if (z->inf_base) (void) hipEventDestroy(z->inf_base);
	delete z;
}

extern "C" size_t ngm_bgzf_bound(size_t n) { return n + 64 * ((n + ngm::bgzf::kIn - 1) / ngm::bgzf::kIn) + 64; }

extern "C" float ngm_bgzf_last_kernel_ms(const ngm_bgzf *z) { return z ? z->last_ms : 0.f; }

static long long compress_on_device(ngm_bgzf *z, const uint8_t *d_raw, size_t n, void *out, size_t out_cap);

extern "C" long long ngm_bgzf_compress(ngm_bgzf *z, const void *raw, size_t n, void *out, size_t out_cap) {
	if (!z || (!raw && n) || !out) { ngm::pipeline_set_error("ngm_bgzf_compress: bad arguments"); return -22; }
	if (n == 0) return 0;
	BGZF_HIP_TRY(hipSetDevice(z->device));
	if (n + 16 > z->d_raw.cap) NGM_MEM_TRY(z->d_raw.alloc(n + n / 4 + 4096));
	BGZF_HIP_TRY(hipMemcpyAsync(z->d_raw.p, raw, n, hipMemcpyHostToDevice, z->st));
	return compress_on_device(z, z->d_raw.p, n, out, out_cap);
}

// the same for bytes that already are in this device's memory (complete: the caller has synchronised the stream that wrote them)
extern "C" long long ngm_bgzf_compress_device(ngm_bgzf *z, const void *d_raw, size_t n, void *out, size_t out_cap) {
	if (!z || (!d_raw && n) || !out) { ngm::pipeline_set_error("ngm_bgzf_compress_device: bad arguments"); return -22; }
	if (n == 0) return 0;
	BGZF_HIP_TRY(hipSetDevice(z->device));
	return compress_on_device(z, (const uint8_t *) d_raw, n, out, out_cap);
}

static long long compress_on_device(ngm_bgzf *z, const uint8_t *d_raw, size_t n, void *out, size_t out_cap) {
	if (out_cap < ngm_bgzf_bound(n)) { ngm::pipeline_set_error("ngm_bgzf_compress: the output buffer holds %zu bytes, %zu may be needed", out_cap, ngm_bgzf_bound(n)); return -22; }
	const size_t nb = (n + ngm::bgzf::kIn - 1) / ngm::bgzf::kIn;
	if (nb > 0x7fffffffull) { ngm::pipeline_set_error("ngm_bgzf_compress: too much input for one call"); return -22; }
	const size_t blocks = nb + nb / 4 + 16;
	if (nb > z->d_offsets.cap) {
		z->d_out.release(); z->d_sizes.release(); z->d_offsets.release();   // (the whole group first: after a refusal nothing of it is left, and the next call asks again)
		NGM_MEM_TRY(z->d_out.alloc(blocks * ngm::bgzf::kStride));
		NGM_MEM_TRY(z->d_sizes.alloc(blocks));
		NGM_MEM_TRY(z->d_offsets.alloc(blocks));
	}
	if (nb > z->h_offsets.cap) {
		z->h_sizes.release(); z->h_offsets.release();
		NGM_MEM_TRY(z->h_sizes.alloc(blocks));
		NGM_MEM_TRY(z->h_offsets.alloc(blocks));
	}
	ngm::bgzf::Args A{};
	A.raw = d_raw; A.n = n; A.n_blocks = (int) nb; A.out = z->d_out.p; A.sizes = z->d_sizes.p; A.scratch = z->d_scratch.p;
	A.crc_table = (const uint32_t *) (z->d_tables.p + kTabCrc); A.xpow = (const uint32_t *) (z->d_tables.p + kTabXpow);
	A.len_code = z->d_tables.p + kTabLen; A.dist_code = z->d_tables.p + kTabDist;
	A.phase_cycles = z->d_phases.p;
	if (z->d_phases.p) BGZF_HIP_TRY(hipMemsetAsync(z->d_phases.p, 0, 64, z->st));
	BGZF_HIP_TRY(hipEventRecord(z->ev0, z->st));
	hipLaunchKernelGGL(ngm::bgzf::deflate_kernel, dim3((unsigned) std::min<size_t>(nb, (size_t) z->grid)), dim3(ngm::bgzf::kNT), ngm::bgzf::deflate_lds_bytes(), z->st, A);
	BGZF_HIP_TRY(hipGetLastError());
	BGZF_HIP_TRY(hipEventRecord(z->ev1, z->st));
	BGZF_HIP_TRY(hipMemcpyAsync(z->h_sizes.p, z->d_sizes.p, nb * 4, hipMemcpyDeviceToHost, z->st));
	BGZF_HIP_TRY(hipStreamSynchronize(z->st));
	unsigned long long total = 0;
	for (size_t b = 0; b < nb; ++b) {
		if (z->h_sizes.p[b] < 26u + 2u || z->h_sizes.p[b] > (uint32_t) ngm::bgzf::kStride) { ngm::pipeline_set_error("GPU BGZF compressor: block %zu has %u bytes", b, z->h_sizes.p[b]); return -5; }
		z->h_offsets.p[b] = total;
		total += z->h_sizes.p[b];
	}
	if (total > out_cap) { ngm::pipeline_set_error("GPU BGZF compressor: %llu bytes for a buffer of %zu", total, out_cap); return -5; }
	if (total + 16 > z->d_dense.cap) NGM_MEM_TRY(z->d_dense.alloc((size_t) total + (size_t) total / 4 + 4096));
	BGZF_HIP_TRY(hipMemcpyAsync(z->d_offsets.p, z->h_offsets.p, nb * 8, hipMemcpyHostToDevice, z->st));
	hipLaunchKernelGGL(ngm::bgzf::gather_kernel, dim3((unsigned) std::min<size_t>(nb, (size_t) z->grid * 8)), dim3(256), 0, z->st, (const uint8_t *) z->d_out.p, (const uint32_t *) z->d_sizes.p,
			(const unsigned long long *) z->d_offsets.p, z->d_dense.p, (int) nb);
	BGZF_HIP_TRY(hipGetLastError());
	BGZF_HIP_TRY(hipMemcpyAsync(out, z->d_dense.p, (size_t) total, hipMemcpyDeviceToHost, z->st));
	BGZF_HIP_TRY(hipStreamSynchronize(z->st));
	if (z->d_phases.p) {
		unsigned long long ph[8];
		BGZF_HIP_TRY(hipMemcpy(ph, z->d_phases.p, 64, hipMemcpyDeviceToHost));
		fprintf(stderr, "[ngm-hip] BGZF kernel, us of thread 0 per block (100 MHz clock): load %.1f | matching %.1f | crc + histograms %.1f | code lengths + codes %.1f | header + match scan %.1f | token bits %.1f | emit + copy out %.1f\n",
				ph[0] / 100.0 / nb, ph[1] / 100.0 / nb, ph[2] / 100.0 / nb, ph[3] / 100.0 / nb, ph[4] / 100.0 / nb, ph[5] / 100.0 / nb, ph[6] / 100.0 / nb);
	}
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, z->ev0, z->ev1) == hipSuccess) z->last_ms = ms;
	return (long long) total;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------
extern "C" size_t ngm_bgzf_inflated_size(const void *members, size_t n) {
	size_t total = 0;
	if (!members || !ngm::inflate::walk_members((const uint8_t *) members, n, nullptr, &total)) return (size_t) -1;
	return total;
}

namespace {
constexpr size_t kInfChunkIn = (size_t) 16 << 20, kInfChunkOut = (size_t) 64 << 20;   // a chunk ends before it would pass either

int inflate_setup(ngm_bgzf *z) {
	if (z->inf_ready) return 0;
	const std::vector<uint32_t> t = ngm::inflate::crc_tables();
	NGM_MEM_TRY(z->d_inf_tables.alloc(t.size()));
	BGZF_HIP_TRY(hipMemcpy(z->d_inf_tables.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
	// more than 64 KiB of LDS per workgroup: the attribute is set for this object's device, and its result counts
	BGZF_HIP_TRY(hipFuncSetAttribute((const void *) ngm::inflate::inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ngm::inflate::inflate_lds_bytes()));
	for (ngm_bgzf::InflateSlot &s : z->inf) {
		BGZF_HIP_TRY(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
		BGZF_HIP_TRY(hipEventCreate(&s.ev0));
		BGZF_HIP_TRY(hipEventCreate(&s.ev1));
	}
	BGZF_HIP_TRY(hipEventCreate(&z->inf_base));
	z->inf_ready = true;
	return 0;
}

int inflate_reserve(ngm_bgzf::InflateSlot &s, size_t in_bytes, size_t out_bytes, size_t members) {
	if (in_bytes > s.h_in.cap) {
		s.d_in.release(); s.h_in.release();
		NGM_MEM_TRY(s.d_in.alloc(in_bytes));
		NGM_MEM_TRY(s.h_in.alloc(in_bytes));
	}
	if (out_bytes > s.h_out.cap) {
		s.d_out.release(); s.h_out.release();
		NGM_MEM_TRY(s.d_out.alloc(out_bytes));
		NGM_MEM_TRY(s.h_out.alloc(out_bytes));
	}
	if (members > s.h_status.cap) {
		s.d_mem.release(); s.d_status.release(); s.h_mem.release(); s.h_status.release();
		NGM_MEM_TRY(s.d_mem.alloc(members));
		NGM_MEM_TRY(s.h_mem.alloc(members));
		NGM_MEM_TRY(s.d_status.alloc(members));
		NGM_MEM_TRY(s.h_status.alloc(members));
	}
	return 0;
}

// waits for the slot's chunk, adds its kernel time, looks at its status words and moves its text to its place; *bad: the first refused member.
// last_ms is the time during which an inflate kernel ran: the two slots' kernels are on two streams and may overlap on the device, so the
// chunks' intervals [ev0, ev1] are united (measured from inf_base, harvested in chunk order), not summed.
int inflate_harvest(ngm_bgzf *z, ngm_bgzf::InflateSlot &s, uint8_t *out, long long *bad, uint32_t *bad_status) {
	if (!s.busy) return 0;
	s.busy = false;
	BGZF_HIP_TRY(hipStreamSynchronize(s.st));
	float t0 = 0.f, t1 = 0.f;
	if (hipEventElapsedTime(&t0, z->inf_base, s.ev0) == hipSuccess && hipEventElapsedTime(&t1, z->inf_base, s.ev1) == hipSuccess) {
		if (t1 > std::max(t0, z->inf_busy_until)) z->last_ms += t1 - std::max(t0, z->inf_busy_until);
		z->inf_busy_until = std::max(z->inf_busy_until, t1);
	}
	for (size_t m = 0; m < s.n_members; ++m) if (s.h_status.p[m] != ngm::inflate::kOk) {
		if (*bad < 0) { *bad = (long long) (s.first_member + m); *bad_status = s.h_status.p[m]; }
		return 0;
	}
	if (*bad < 0) memcpy(out + s.text_at, s.h_out.p, s.text_bytes);
	return 0;
}
}  // namespace

extern "C" long long ngm_bgzf_inflate(ngm_bgzf *z, const void *members, size_t n, void *out, size_t out_cap) {
	if (!z || (!members && n) || (!out && out_cap)) { ngm::pipeline_set_error("ngm_bgzf_inflate: bad arguments"); return -22; }
	const uint8_t *in = (const uint8_t *) members;
	std::vector<ngm::inflate::HostMember> chain;
	size_t total = 0;
	if (!ngm::inflate::walk_members(in, n, &chain, &total)) { ngm::pipeline_set_error("ngm_bgzf_inflate: the data is not a run of whole BGZF members"); return -22; }
	if (total > out_cap) { ngm::pipeline_set_error("ngm_bgzf_inflate: %zu bytes of text for a buffer of %zu", total, out_cap); return -22; }
	z->last_ms = 0.f;
	if (chain.empty()) return 0;
	BGZF_HIP_TRY(hipSetDevice(z->device));
	if (int rc = inflate_setup(z)) return rc;
	long long bad = -1;
	uint32_t bad_status = 0;
	size_t m0 = 0, text_at = 0;
	for (int c = 0; m0 < chain.size() && bad < 0; ++c) {
		// the members of this chunk: at least one, then as many as stay inside both limits
		size_t m1 = m0, in_bytes = 0, out_bytes = 0;
		while (m1 < chain.size() && (m1 == m0 || (in_bytes + chain[m1].size <= kInfChunkIn && out_bytes + chain[m1].isize <= kInfChunkOut))) {
			in_bytes += chain[m1].size; out_bytes += chain[m1].isize; ++m1;
		}
		ngm_bgzf::InflateSlot &s = z->inf[c & 1];
		if (int rc = inflate_harvest(z, s, (uint8_t *) out, &bad, &bad_status)) return rc;
		if (bad >= 0) break;
		const bool whole = m0 == 0 && m1 == chain.size();   // (a small input takes what it needs, a large one whole chunks)
		if (int rc = inflate_reserve(s, whole ? in_bytes + 64 : kInfChunkIn + 65536 + 64, whole ? out_bytes + 64 : kInfChunkOut + 65536 + 64, whole ? m1 - m0 : std::max<size_t>(m1 - m0, kInfChunkIn / 28 / 64))) return rc;
		const size_t base = chain[m0].at;
		memcpy(s.h_in.p, in + base, in_bytes);
		size_t o = 0;
		for (size_t m = m0; m < m1; ++m) {
			const ngm::inflate::HostMember &h = chain[m];
			s.h_mem.p[m - m0] = ngm::inflate::Member{(uint32_t) (h.at - base + h.payload), (uint32_t) (h.at - base + h.size - 8), (uint32_t) o, h.isize};
			o += h.isize;
		}
		s.first_member = m0; s.n_members = m1 - m0; s.text_at = text_at; s.text_bytes = out_bytes;
		BGZF_HIP_TRY(hipMemcpyAsync(s.d_in.p, s.h_in.p, in_bytes, hipMemcpyHostToDevice, s.st));
		BGZF_HIP_TRY(hipMemcpyAsync(s.d_mem.p, s.h_mem.p, s.n_members * sizeof(ngm::inflate::Member), hipMemcpyHostToDevice, s.st));
		ngm::inflate::Args A{};
		A.in = s.d_in.p; A.members = s.d_mem.p; A.n_members = (int) s.n_members; A.out = s.d_out.p; A.status = s.d_status.p;
		A.crc_table = z->d_inf_tables.p; A.xpow = z->d_inf_tables.p + 256;
		if (c == 0) { BGZF_HIP_TRY(hipEventRecord(z->inf_base, s.st)); z->inf_busy_until = 0.f; }
		BGZF_HIP_TRY(hipEventRecord(s.ev0, s.st));
		hipLaunchKernelGGL(ngm::inflate::inflate_kernel, dim3((unsigned) std::min<size_t>(s.n_members, (size_t) z->grid * 2)), dim3(ngm::inflate::kNT), ngm::inflate::inflate_lds_bytes(), s.st, A);
		BGZF_HIP_TRY(hipGetLastError());
		BGZF_HIP_TRY(hipEventRecord(s.ev1, s.st));
		BGZF_HIP_TRY(hipMemcpyAsync(s.h_status.p, s.d_status.p, s.n_members * 4, hipMemcpyDeviceToHost, s.st));
		if (out_bytes) BGZF_HIP_TRY(hipMemcpyAsync(s.h_out.p, s.d_out.p, out_bytes, hipMemcpyDeviceToHost, s.st));
		s.busy = true;
		text_at += out_bytes;
		m0 = m1;
	}
	// what is still in flight, in chunk order: the slot of the chunk before the last one first
	const int chunks_done = (int) ((z->inf[0].busy ? 1 : 0) + (z->inf[1].busy ? 1 : 0));
	if (chunks_done == 2) {
		const int older = z->inf[0].first_member < z->inf[1].first_member ? 0 : 1;
		if (int rc = inflate_harvest(z, z->inf[older], (uint8_t *) out, &bad, &bad_status)) return rc;
		if (int rc = inflate_harvest(z, z->inf[older ^ 1], (uint8_t *) out, &bad, &bad_status)) return rc;
	} else {
		for (ngm_bgzf::InflateSlot &s : z->inf) if (int rc = inflate_harvest(z, s, (uint8_t *) out, &bad, &bad_status)) return rc;
	}
	if (bad >= 0) { ngm::pipeline_set_error("GPU BGZF inflate: member %lld refused (status %u)", bad, bad_status); return -74; }
	return (long long) total;
}
