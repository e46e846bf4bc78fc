// buffer_driver.cpp -- ngm::Owned (nextgenmap_amd/csrc/buffer.h) over a counting malloc, for tests/test_buffer_host.py: the three growth
// rules' capacities and requests, the fall-back of reserve, moves and swaps, an early return.  Stand-alone, built with
// -fsanitize=address,undefined; it ends with nothing live, exit status 0, and the sanitizer's leak check at exit agrees.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>
#include <utility>

#include "../../nextgenmap_amd/csrc/buffer.h"

namespace {

// malloc, counted: live bytes, requests and frees so far, the size of the last request; bit i of fail_mask refuses the i-th request from
// now; a block comes back with the bytes it was asked with, or the driver ends
struct CountingMem {
	static inline size_t live = 0, gets = 0, puts = 0, last_bytes = 0;
	static inline unsigned fail_mask = 0;
	static inline std::map<void *, size_t> bytes_of;
	static void *get(size_t bytes) {
		++gets;
		last_bytes = bytes;
		const bool fail = fail_mask & 1u;
		fail_mask >>= 1;
		if (fail) return nullptr;
		void *p = malloc(bytes);
		if (!p) return nullptr;
		bytes_of[p] = bytes;
		live += bytes;
		return p;
	}
	static void put(void *p, size_t bytes) {
		auto it = bytes_of.find(p);
		if (it == bytes_of.end()) { printf("put of a block that is not live\n"); exit(3); }
		if (it->second != bytes) { printf("put of %zu bytes for a block of %zu\n", bytes, it->second); exit(4); }
		live -= it->second;
		bytes_of.erase(it);
		++puts;
		free(p);
	}
};

template <typename T> using B = ngm::Owned<T, CountingMem>;

static_assert(!std::is_copy_constructible<B<uint32_t>>::value, "a buffer has one owner");
static_assert(!std::is_copy_assignable<B<uint32_t>>::value, "a buffer has one owner");
static_assert(std::is_nothrow_move_constructible<B<uint32_t>>::value && std::is_nothrow_move_assignable<B<uint32_t>>::value, "ownership moves");

// "<rule> <type> <n> <return> <capacity> <bytes of the last request> <p set>", each from an empty buffer
template <typename T>
void capacities(const char *type, size_t big) {
	const size_t ns[] = {0, 1, 7, 8, 9, 63, 64, 1000, big};
	for (size_t n : ns) {
		for (int rule = 0; rule < 3; ++rule) {
			B<T> b;
			CountingMem::last_bytes = 0;
			const int rc = rule == 0 ? b.reserve(n) : rule == 1 ? b.alloc(n) : b.grow(n);
			printf("%s %s %zu %d %zu %zu %d\n", rule == 0 ? "reserve" : rule == 1 ? "alloc" : "grow", type, n, rc, b.cap, CountingMem::last_bytes, b.p ? 1 : 0);
		}
	}
}

int three_buffers_early_return(bool early) {
	B<uint32_t> a, b, c;
	if (a.reserve(100) || b.reserve(200)) return -12;
	if (early) return -5;   // (as a HIP call that failed behind two reserves)
	if (c.reserve(300)) return -12;
	return 0;
}

}  // namespace

int main() {
	capacities<uint8_t>("u8", (size_t) 536870920);
	capacities<uint64_t>("u64", (size_t) 67108872);
	printf("live %zu\n", CountingMem::live);

	{   // reserve keeps what fits, frees what does not before it asks again
		B<uint32_t> b;
		b.reserve(100);
		const uint32_t *p0 = b.p;
		size_t g0 = CountingMem::gets;
		b.reserve(112);
		printf("fits %zu %d %zu\n", b.cap, b.p == p0 ? 1 : 0, CountingMem::gets - g0);
		g0 = CountingMem::gets;
		const size_t f0 = CountingMem::puts;
		b.reserve(113);
		printf("regrown %zu %zu %zu %zu\n", b.cap, CountingMem::gets - g0, CountingMem::puts - f0, CountingMem::live);
		b.grow(100);
		printf("grow_fits %zu\n", b.cap);
		b.grow(200);
		printf("grow_regrown %zu %zu\n", b.cap, CountingMem::live);
		b.alloc(3);
		printf("alloc_shrinks %zu %zu\n", b.cap, CountingMem::live);
	}
	{   // the first request refused: exactly n; both refused: nothing, and the old block is gone
		B<uint32_t> b;
		size_t g0 = CountingMem::gets;
		CountingMem::fail_mask = 1;
		int rc = b.reserve(1000);
		printf("fallback %d %zu %zu %zu\n", rc, b.cap, CountingMem::gets - g0, CountingMem::last_bytes);
		CountingMem::fail_mask = 3;
		rc = b.reserve(2000);
		printf("both_fail %d %d %zu %zu\n", rc, b.p ? 1 : 0, b.cap, CountingMem::live);
		CountingMem::fail_mask = 1;
		rc = b.alloc(10);
		printf("alloc_fail %d %d %zu\n", rc, b.p ? 1 : 0, b.cap);
		CountingMem::fail_mask = 1;
		rc = b.grow(10);
		printf("grow_fail %d %d %zu %zu\n", rc, b.p ? 1 : 0, b.cap, CountingMem::live);
	}
	{   // moves and swaps: one owner at a time, the old block of an assignment's target freed exactly once
		B<uint32_t> a;
		a.reserve(10);
		const uint32_t *pa = a.p;
		B<uint32_t> b(std::move(a));
		printf("move_ctor %d %zu %d %zu %zu\n", a.p ? 1 : 0, a.cap, b.p == pa ? 1 : 0, b.cap, CountingMem::live);
		B<uint32_t> c;
		c.alloc(5);
		const size_t f0 = CountingMem::puts;
		c = std::move(b);
		printf("move_assign %zu %d %zu %d %zu %zu\n", CountingMem::puts - f0, c.p == pa ? 1 : 0, c.cap, b.p ? 1 : 0, b.cap, CountingMem::live);
		B<uint32_t> d;
		d.alloc(3);
		const uint32_t *pd = d.p;
		const size_t g1 = CountingMem::gets, f1 = CountingMem::puts;
		std::swap(c, d);
		printf("swap %d %zu %d %zu %zu %zu\n", c.p == pd ? 1 : 0, c.cap, d.p == pa ? 1 : 0, d.cap, CountingMem::gets - g1, CountingMem::puts - f1);
		B<uint32_t> &same = d;
		d = std::move(same);
		printf("self_move %d %zu %zu %zu\n", d.p == pa ? 1 : 0, d.cap, CountingMem::puts - f1, CountingMem::live);
	}
	printf("scope_end %zu\n", CountingMem::live);
	int rc = three_buffers_early_return(true);
	printf("early_return %d %zu\n", rc, CountingMem::live);
	rc = three_buffers_early_return(false);
	printf("full_return %d %zu\n", rc, CountingMem::live);
	printf("end %zu %zu %zu\n", CountingMem::live, CountingMem::gets, CountingMem::puts);
	return CountingMem::live == 0 && CountingMem::bytes_of.empty() ? 0 : 1;
}
