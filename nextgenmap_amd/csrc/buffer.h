// buffer.h -- the one owner of device and pinned host memory: ngm::Owned<T, Mem>.  No HIP here: where the memory comes from is the policy
// `Mem` (static void *get(size_t bytes), null: no memory; static void put(void *, size_t bytes), with the bytes get was asked for).  The
// two HIP policies and the names DevBuf, PinnedBuf and Buf are in device_mem.h; tests/cpp/buffer_driver.cpp runs this header over a
// counting malloc.
// The destructor frees, a move hands the block on, there is no copy: a buffer that is a member or a local needs no release list and leaks
// on no return path.  release() is for the places that free early on purpose (peak memory of an index build).
#pragma once

#include <algorithm>
#include <cstddef>

namespace ngm {

template <typename T, typename Mem>
struct Owned {
	T *p = nullptr;
	size_t cap = 0;   // elements the holder may use (alloc(0): one element is asked for, cap stays 0).  Holders read p and cap and never write
	                  // them: release() works out from cap how many bytes were asked for (buffer_driver.cpp checks it on every put)

	Owned() = default;
	Owned(const Owned &) = delete;
	Owned &operator=(const Owned &) = delete;
	Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	Owned &operator=(Owned &&o) noexcept {
		if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
		return *this;
	}
	~Owned() { release(); }

	void release() { if (p) Mem::put(p, std::max<size_t>(cap, 1) * sizeof(T)); p = nullptr; cap = 0; }   // (alloc(0) asked for one element)

	// room for n elements, kept when it is there: an eighth more than asked for (batches of a real run differ by a few per cent, and every
	// new maximum would otherwise be a free + allocation -- two device-wide synchronisations -- in the middle of the mapping pass), at
	// most 64 MB more (the index arrays come through here too); exactly n where that much is not to be had
	int reserve(size_t n) {
		if (n <= cap) return 0;
		release();
		const size_t want = n + std::min<size_t>(n / 8, ((size_t) 64 << 20) / sizeof(T));
		if (take(want, want)) return 0;
		return take(n, n) ? 0 : -1;
	}
	// exactly n elements, whatever was there before
	int alloc(size_t n) { release(); return take(std::max<size_t>(n, 1), n) ? 0 : -1; }
	// room for n elements, kept when it is there, with a quarter to spare when it has to grow
	int grow(size_t n) { return n <= cap ? 0 : alloc(n + n / 4 + 64); }

private:
	bool take(size_t elements, size_t cap_) {
		p = static_cast<T *>(Mem::get(elements * sizeof(T)));
		if (p) cap = cap_;
		return p != nullptr;
	}
};

}  // namespace ngm
