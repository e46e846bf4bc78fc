// bgzf_inflate_device.h -- BGZF members inflated on the GPU: one workgroup per member, a persistent grid over the members.
//
// A BGZF file (every BAM, every file written by bgzip) is a chain of independent gzip members of at most 64 KiB of text each.  The host
// walks the chain (walk_members below: BSIZE from the BC subfield, ISIZE from the trailer) and hands the kernel one descriptor per
// member; the kernel inflates the member into LDS, checks length and CRC-32 against the trailer and copies the text to its place in the
// output.  Whatever the stream says:
//   * the bit reader (Bits) never loads a byte at or behind `end`, the first byte of the member's trailer;
//   * every byte written is checked against the member's ISIZE (<= 65536, the size of the LDS stage);
//   * every match distance is checked against the bytes this member has produced so far;
//   * a symbol whose bits lie behind `end` ends the loop (kInputOverrun).
// A refused member gets a non-zero status word; nothing traps.
//
// The decoder itself (Bits, construct, decode, inflate_member, crc_part, copy_out) is __host__ __device__: tests/cpp/bam_input_driver.cpp
// runs these very functions on the CPU (cooperative steps with a loop over the thread index) under AddressSanitizer, where damaged
// streams are tried first.
//
// Organisation: thread 0 of the workgroup decodes the symbols and copies the matches inside LDS (one dependent table lookup per symbol
// is the critical path; the other threads wait at the barrier and take no issue slots); all threads then compute the CRC-32 (a chunk
// each, combined with the x^(8 m) table as in bgzf_device.h) and copy the text out with dword stores.
// LDS per workgroup: 65536 (text) + sizeof(Tables) (4192) + 1024 (CRC table) + 16 = 70768 bytes -> two workgroups per CU of 160 KiB.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define NGM_INF_HD __host__ __device__ inline
#else
#define NGM_INF_HD inline
#endif

namespace ngm {
namespace inflate {

constexpr int kLitBits = 10, kDistBits = 8;   // codes up to this length take one table lookup, longer ones the canonical walk
constexpr uint32_t kMaxIsize = 65536;
constexpr int kNT = 256;

enum Status : uint32_t {
	kOk = 0, kBadBlockType = 1, kBadStored = 2, kBadCodeLengths = 3, kBadLitSet = 4, kBadDistSet = 5, kBadSymbol = 6, kBadDistance = 7,
	kOutputOverrun = 8, kInputOverrun = 9, kLengthMismatch = 10, kCrcMismatch = 11, kNoEndOfBlock = 12, kTrailingBytes = 13
};

// one member of a run of members: offsets into the run / into the run's text
struct Member {
	uint32_t payload;   // first byte of the DEFLATE stream
	uint32_t end;       // first byte of the trailer (CRC-32, ISIZE)
	uint32_t out_off;   // where the member's text goes
	uint32_t isize;     // the trailer's ISIZE (<= kMaxIsize: checked by the host)
};

// a canonical Huffman code: symbols ordered by code length, then by value (RFC 1951 3.2.2)
struct Huff {
	uint16_t count[16];
	uint16_t symbol[288];
};
struct Tables {   // 4192 bytes
	uint16_t lit_fast[1 << kLitBits];    // symbol << 4 | code length; 0: the code is longer than the table's bits (or invalid)
	uint16_t dist_fast[1 << kDistBits];
	Huff lit, dist;
	uint16_t offs[16], next[16];
	uint8_t lens[320];
	uint8_t pre_lens[32];
};

static_assert(sizeof(Tables) == 4192, "the LDS budget in the header comment and in DESIGN.md");

struct Bits {
	const uint8_t *in;
	uint32_t pos, end;   // next byte to load; one past the last byte that may be loaded
	uint64_t buf;
	int cnt;             // valid bits in buf; the bits above them are zero
	// > 32 bits unless the input ends: byte loads up to a 4-byte boundary, whole words from there, bytes again at the end
	NGM_INF_HD void refill() {
		while (cnt <= 32 && pos < end) {
			const uint8_t *a = in + pos;
			if (((uintptr_t) a & 3u) == 0 && end - pos >= 4) {
				uint32_t w;
				__builtin_memcpy(&w, __builtin_assume_aligned(a, 4), 4);
				buf |= (uint64_t) w << cnt;
				cnt += 32; pos += 4;
			} else {
				buf |= (uint64_t) *a << cnt;
				cnt += 8; pos += 1;
			}
		}
	}
	NGM_INF_HD bool need(int n) { if (cnt < n) refill(); return cnt >= n; }
	NGM_INF_HD uint32_t take(int n) { const uint32_t v = (uint32_t) (buf & ((1ull << n) - 1ull)); buf >>= n; cnt -= n; return v; }
};

NGM_INF_HD uint32_t reverse_bits(uint32_t v, int n) {
	uint32_t r = 0;
	for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
	return r;
}

// Builds the code of `n` lengths.  Returns zlib's verdict (inflate_table): false for an over-subscribed set, and for an incomplete one
// unless it is a literal/length or distance set whose longest code has one bit (a single distance code is legal).  No code at all is
// accepted here: whoever decodes with it finds no symbol.
NGM_INF_HD bool construct(Tables &T, Huff &h, uint16_t *fast, int fast_bits, const uint8_t *lens, int n, bool code_lengths) {
	for (int l = 0; l < 16; ++l) h.count[l] = 0;
	for (int s = 0; s < n; ++s) h.count[lens[s] & 15]++;
	for (int i = 0; i < (1 << fast_bits); ++i) fast[i] = 0;
	if (h.count[0] == n) return true;
	int left = 1, longest = 0;
	for (int l = 1; l <= 15; ++l) {
		left = (left << 1) - (int) h.count[l];
		if (left < 0) return false;
		if (h.count[l]) longest = l;
	}
	if (left > 0 && (code_lengths || longest != 1)) return false;
	uint32_t code = 0;
	T.offs[1] = 0; T.next[0] = 0;
	for (int l = 1; l <= 15; ++l) {
		code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
		T.next[l] = (uint16_t) code;   // (< 2^15 for every length that has a code: the set is not over-subscribed)
		if (l < 15) T.offs[l + 1] = (uint16_t) (T.offs[l] + h.count[l]);
	}
	for (int s = 0; s < n; ++s) {
		const int l = lens[s] & 15;
		if (!l) continue;
		h.symbol[T.offs[l]++] = (uint16_t) s;
		const uint32_t c = T.next[l]++;
		if (l <= fast_bits) for (uint32_t i = reverse_bits(c, l); i < (1u << fast_bits); i += 1u << l) fast[i] = (uint16_t) ((s << 4) | l);
	}
	return true;
}

// the next symbol, or -1 (no code of the set matches the next bits) / -2 (its bits lie behind the end of the input)
NGM_INF_HD int decode(Bits &b, const Huff &h, const uint16_t *fast, int fast_bits) {
	b.refill();
	const uint32_t e = fast[b.buf & ((1u << fast_bits) - 1u)];
	if (e & 15u) {
		if ((int) (e & 15u) > b.cnt) return -2;
		b.take((int) (e & 15u));
		return (int) (e >> 4);
	}
	int code = 0, first = 0, index = 0;
	for (int len = 1; len <= 15; ++len) {
		code |= (int) ((b.buf >> (len - 1)) & 1u);
		const int cnt = h.count[len];
		if (code - cnt < first) {
			if (len > b.cnt) return -2;
			b.take(len);
			return h.symbol[index + (code - first)];
		}
		index += cnt; first += cnt;
		first <<= 1; code <<= 1;
	}
	return -1;
}

// One member: the DEFLATE stream in[pos, end) -> out[0, isize).  Run by ONE thread.  *produced: the bytes written.
NGM_INF_HD uint32_t inflate_member(const uint8_t *in, uint32_t pos, uint32_t end, uint8_t *out, uint32_t isize, Tables &T, uint32_t *produced) {
	const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	Bits b;
	b.in = in; b.pos = pos; b.end = end; b.buf = 0; b.cnt = 0;
	uint32_t outn = 0;
	*produced = 0;
	if (isize > kMaxIsize) return kLengthMismatch;
	for (;;) {
		if (!b.need(3)) return kInputOverrun;
		const uint32_t final_block = b.take(1), type = b.take(2);
		if (type == 0) {
			// stored: back to a byte boundary; the whole bytes still in the bit buffer go back to the input
			b.take(b.cnt & 7);
			b.pos -= (uint32_t) (b.cnt >> 3);
			b.buf = 0; b.cnt = 0;
			if (b.end - b.pos < 4) return kInputOverrun;
			const uint32_t len = (uint32_t) in[b.pos] | ((uint32_t) in[b.pos + 1] << 8), nlen = (uint32_t) in[b.pos + 2] | ((uint32_t) in[b.pos + 3] << 8);
			b.pos += 4;
			if ((len ^ nlen) != 0xFFFFu) return kBadStored;
			if (b.end - b.pos < len) return kInputOverrun;
			if (isize - outn < len) return kOutputOverrun;
			for (uint32_t i = 0; i < len; ++i) out[outn + i] = in[b.pos + i];
			outn += len; b.pos += len;
		} else if (type == 1 || type == 2) {
			if (type == 1) {
				for (int i = 0; i < 144; ++i) T.lens[i] = 8;
				for (int i = 144; i < 256; ++i) T.lens[i] = 9;
				for (int i = 256; i < 280; ++i) T.lens[i] = 7;
				for (int i = 280; i < 288; ++i) T.lens[i] = 8;
				for (int i = 0; i < 32; ++i) T.lens[288 + i] = 5;
				(void) construct(T, T.lit, T.lit_fast, kLitBits, T.lens, 288, false);
				(void) construct(T, T.dist, T.dist_fast, kDistBits, T.lens + 288, 32, false);
			} else {
				if (!b.need(14)) return kInputOverrun;
				const int hlit = (int) b.take(5) + 257, hdist = (int) b.take(5) + 1, hclen = (int) b.take(4) + 4;
				if (hlit > 286 || hdist > 30) return kBadCodeLengths;
				for (int i = 0; i < 19; ++i) T.pre_lens[i] = 0;
				for (int i = 0; i < hclen; ++i) {
					if (!b.need(3)) return kInputOverrun;
					T.pre_lens[order[i]] = (uint8_t) b.take(3);
				}
				// (the code-length code borrows the distance set's tables: they are built after it has been used)
				if (!construct(T, T.dist, T.dist_fast, 7, T.pre_lens, 19, true)) return kBadCodeLengths;
				const int total = hlit + hdist;
				int i = 0;
				while (i < total) {
					const int s = decode(b, T.dist, T.dist_fast, 7);
					if (s < 0) return s == -2 ? kInputOverrun : kBadCodeLengths;
					if (s < 16) { T.lens[i++] = (uint8_t) s; continue; }
					int rep;
					uint8_t v = 0;
					if (s == 16) { if (i == 0) return kBadCodeLengths; if (!b.need(2)) return kInputOverrun; v = T.lens[i - 1]; rep = 3 + (int) b.take(2); }
					else if (s == 17) { if (!b.need(3)) return kInputOverrun; rep = 3 + (int) b.take(3); }
					else { if (!b.need(7)) return kInputOverrun; rep = 11 + (int) b.take(7); }
					if (i + rep > total) return kBadCodeLengths;
					for (int k = 0; k < rep; ++k) T.lens[i++] = v;
				}
				if (T.lens[256] == 0) return kNoEndOfBlock;
				if (!construct(T, T.lit, T.lit_fast, kLitBits, T.lens, hlit, false)) return kBadLitSet;
				if (!construct(T, T.dist, T.dist_fast, kDistBits, T.lens + hlit, hdist, false)) return kBadDistSet;
			}
			for (;;) {
				int s = decode(b, T.lit, T.lit_fast, kLitBits);
				if (s < 0) return s == -2 ? kInputOverrun : kBadSymbol;
				if (s < 256) {
					if (outn >= isize) return kOutputOverrun;
					out[outn++] = (uint8_t) s;
					continue;
				}
				if (s == 256) break;
				s -= 257;
				if (s > 28) return kBadSymbol;
				const int leb = (s < 8 || s == 28) ? 0 : (s - 4) >> 2;
				uint32_t len = s < 8 ? 3u + (uint32_t) s : s == 28 ? 258u : 3u + ((4u + ((uint32_t) s & 3u)) << leb);
				if (!b.need(leb)) return kInputOverrun;
				len += b.take(leb);
				const int d = decode(b, T.dist, T.dist_fast, kDistBits);
				if (d < 0) return d == -2 ? kInputOverrun : kBadSymbol;
				if (d > 29) return kBadSymbol;
				const int deb = d < 4 ? 0 : (d - 2) >> 1;
				uint32_t dist = d < 4 ? 1u + (uint32_t) d : 1u + ((2u + ((uint32_t) d & 1u)) << deb);
				if (!b.need(deb)) return kInputOverrun;
				dist += b.take(deb);
				if (dist > outn) return kBadDistance;
				if (len > isize - outn) return kOutputOverrun;
				const uint8_t *src = out + outn - dist;
				uint8_t *dst = out + outn;
				for (uint32_t i = 0; i < len; ++i) dst[i] = src[i];
				outn += len;
			}
		} else {
			return kBadBlockType;
		}
		if (final_block) break;
	}
	// the stream ends where the trailer begins (zlib reads the trailer right behind the stream)
	if (b.pos - (uint32_t) (b.cnt >> 3) != end) return kTrailingBytes;
	*produced = outn;
	return outn == isize ? kOk : kLengthMismatch;
}

NGM_INF_HD uint32_t gf_mulmod(uint32_t a, uint32_t b) {   // a * b mod the CRC-32 polynomial, reflected (bit 31 = x^0)
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {
		if (a & (0x80000000u >> i)) p ^= b;
		b = (b >> 1) ^ ((b & 1u) ? 0xedb88320u : 0u);
	}
	return p;
}

// thread tid's share of the CRC-32 of text[0, n): the XOR over all nt threads is the CRC.  crc_t: the byte table; xpow[m] = x^(8 m).
NGM_INF_HD uint32_t crc_part(const uint8_t *text, uint32_t n, int tid, int nt, const uint32_t *crc_t, const uint32_t *xpow) {
	const uint32_t chunk = (n + (uint32_t) nt - 1u) / (uint32_t) nt;
	const uint32_t b0 = (uint32_t) tid * chunk < n ? (uint32_t) tid * chunk : n, b1 = n - b0 < chunk ? n : b0 + chunk;
	uint32_t c = 0;
	for (uint32_t i = b0; i < b1; ++i) c = crc_t[(c ^ text[i]) & 255u] ^ (c >> 8);
	uint32_t part = c ? gf_mulmod(c, xpow[n - b1]) : 0u;
	if (tid == 0) part ^= gf_mulmod(0xFFFFFFFFu, xpow[n]) ^ 0xFFFFFFFFu;
	return part;
}

// thread tid's share of text[0, n) -> dst[0, n): whole words where dst is 4-byte aligned, bytes before and behind them
NGM_INF_HD void copy_out(const uint8_t *text, uint32_t n, uint8_t *dst, int tid, int nt) {
	uint32_t head = (uint32_t) ((4u - ((uintptr_t) dst & 3u)) & 3u);
	if (head > n) head = n;
	const uint32_t words = (n - head) >> 2, tail = head + 4u * words;
	if ((uint32_t) tid < head) dst[tid] = text[tid];
	for (uint32_t w = (uint32_t) tid; w < words; w += (uint32_t) nt) {
		const uint8_t *s = text + head + 4u * w;
		const uint32_t v = (uint32_t) s[0] | ((uint32_t) s[1] << 8) | ((uint32_t) s[2] << 16) | ((uint32_t) s[3] << 24);
		__builtin_memcpy(__builtin_assume_aligned(dst + head + 4u * w, 4), &v, 4);
	}
	if ((uint32_t) tid < n - tail) dst[tail + (uint32_t) tid] = text[tail + (uint32_t) tid];
}

NGM_INF_HD uint32_t load_le32(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24); }

// ---- host: the chain of members -------------------------------------------------------------------------------------
struct HostMember { size_t at, size, payload; uint32_t isize; };   // the member's bytes are [at, at + size); payload: offset of its DEFLATE stream
// false unless z[0, n) is made of whole BGZF members: gzip members with the BC subfield (BSIZE = size - 1), none running past n,
// none with an ISIZE above 65536
// the member at z + at: false unless it is a gzip header with FLG = FEXTRA alone whose extra field holds the BC subfield (anywhere among
// the subfields) and lies inside z[0, n).  *xlen: the extra field's length; *bsize: the BC value (the member's size - 1)
inline bool member_header(const uint8_t *z, size_t n, size_t at, size_t *xlen, size_t *bsize) {
	if (n - at < 28 || z[at] != 0x1f || z[at + 1] != 0x8b || z[at + 2] != 8 || z[at + 3] != 4) return false;
	*xlen = (size_t) z[at + 10] | ((size_t) z[at + 11] << 8);
	if (n - at < 12 + *xlen + 8) return false;
	bool have = false;
	for (size_t x = at + 12, xe = at + 12 + *xlen; x + 4 <= xe;) {
		const size_t sl = (size_t) z[x + 2] | ((size_t) z[x + 3] << 8);
		if (x + 4 + sl > xe) return false;
		if (z[x] == 'B' && z[x + 1] == 'C' && sl == 2) { *bsize = (size_t) z[x + 4] | ((size_t) z[x + 5] << 8); have = true; }
		x += 4 + sl;
	}
	return have;
}
// does the file z[0, n) begin with a BGZF member?  (what sends a .gz input to this decoder; the whole chain is walked before any launch)
inline bool first_member_is_bgzf(const uint8_t *z, size_t n) {
	size_t xlen = 0, bsize = 0;
	return n >= 28 && member_header(z, n, 0, &xlen, &bsize);
}
inline bool walk_members(const uint8_t *z, size_t n, std::vector<HostMember> *out, size_t *text_bytes) {
	size_t at = 0, total = 0;
	while (at < n) {
		size_t xlen = 0, bsize = 0;
		if (!member_header(z, n, at, &xlen, &bsize)) return false;
		const size_t size = bsize + 1;
		if (size < 12 + xlen + 8 || size > n - at) return false;
		const uint32_t isize = load_le32(z + at + size - 4);
		if (isize > kMaxIsize) return false;
		if (out) out->push_back(HostMember{at, size, 12 + xlen, isize});
		total += isize;
		at += size;
	}
	if (text_bytes) *text_bytes = total;
	return true;
}

// the tables crc_part reads, as the kernel gets them: the CRC-32 byte table [256], then x^(8 m) mod the polynomial for m = 0 .. kMaxIsize
inline std::vector<uint32_t> crc_tables() {
	std::vector<uint32_t> t(256 + kMaxIsize + 1);
	for (uint32_t i = 0; i < 256; ++i) {
		uint32_t c = i;
		for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xedb88320u : c >> 1;
		t[i] = c;
	}
	t[256] = 0x80000000u;   // x^0
	for (uint32_t m = 1; m <= kMaxIsize; ++m) t[256 + m] = gf_mulmod(t[256 + m - 1], 0x00800000u);   // * x^8
	return t;
}

#if defined(__HIPCC__)
struct Args {
	const uint8_t *in;          // a run of whole members (4-byte aligned)
	const Member *members;
	int n_members;
	uint8_t *out;
	uint32_t *status;           // one word per member
	const uint32_t *crc_table;  // [256]
	const uint32_t *xpow;       // [kMaxIsize + 1]
};

inline size_t inflate_lds_bytes() { return (size_t) kMaxIsize + sizeof(Tables) + 1024 + 16; }

__global__ __launch_bounds__(kNT) void inflate_kernel(Args A) {
	extern __shared__ uint32_t lds_words[];
	uint8_t *text = (uint8_t *) lds_words;
	Tables &T = *(Tables *) (text + kMaxIsize);
	uint32_t *crc_t = (uint32_t *) (text + kMaxIsize + sizeof(Tables));
	uint32_t *sh = crc_t + 256;   // 0: status, 1: CRC-32 of the text
	const int tid = (int) threadIdx.x;
	crc_t[tid] = A.crc_table[tid];
	for (int m = (int) blockIdx.x; m < A.n_members; m += (int) gridDim.x) {
		const Member M = A.members[m];
		if (tid == 0) {
			uint32_t produced = 0;
			sh[0] = inflate_member(A.in, M.payload, M.end, text, M.isize, T, &produced);
			sh[1] = 0;
		}
		__syncthreads();
		uint32_t st = sh[0];
		if (st == kOk) {
			const uint32_t part = crc_part(text, M.isize, tid, kNT, crc_t, A.xpow);
			if (part) atomicXor(&sh[1], part);
		}
		__syncthreads();
		if (st == kOk) {
			if (sh[1] != load_le32(A.in + M.end)) st = kCrcMismatch;
			else copy_out(text, M.isize, A.out + M.out_off, tid, kNT);
		}
		if (tid == 0) A.status[m] = st;
		__syncthreads();
	}
}
#endif

}  // namespace inflate
}  // namespace ngm
