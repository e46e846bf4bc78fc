// device_mem.h -- where ngm::Owned (buffer.h) gets its memory on this side of HIP: DeviceMem (hipMalloc / hipFree) and PinnedMem
// (hipHostMalloc / hipHostFree), and the buffer names the library uses.  Apart from ngm_host_alloc / ngm_host_free, which hand pinned
// memory to callers, these two policies hold the library's only allocation calls.
// Both count, in relaxed atomics: live bytes and allocation calls so far, read by ngm_debug_live_memory (tests/test_gpu_memory.py).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "buffer.h"

// a buffer (or several joined with ||) that found no memory: reported as the failed allocation call it stands for, -5
#define NGM_MEM_TRY(failed)                                                                     \
	do {                                                                                        \
		if (failed) {                                                                           \
			ngm::pipeline_set_error("%s failed: %s (%s:%d)", #failed, hipGetErrorString(hipErrorOutOfMemory), __FILE__, __LINE__); \
			return -5;                                                                          \
		}                                                                                       \
	} while (0)

namespace ngm {

void pipeline_set_error(const char *fmt, ...);   // refindex.cpp

struct MemCount {
	std::atomic<uint64_t> live{0}, calls{0};
	void took(size_t bytes) { live.fetch_add(bytes, std::memory_order_relaxed); calls.fetch_add(1, std::memory_order_relaxed); }
	void gave(size_t bytes) { live.fetch_sub(bytes, std::memory_order_relaxed); }
};

// (a failed allocation leaves no sticky error behind: hipGetLastError clears it)
struct DeviceMem {
	static inline MemCount count;
	static void *get(size_t bytes) {
		void *p = nullptr;
		if (hipMalloc(&p, bytes) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
		count.took(bytes);
		return p;
	}
	static void put(void *p, size_t bytes) { count.gave(bytes); (void) hipFree(p); }
};
struct PinnedMem {
	static inline MemCount count;
	static void *get(size_t bytes) {
		void *p = nullptr;
		if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
		count.took(bytes);
		return p;
	}
	static void put(void *p, size_t bytes) { count.gave(bytes); (void) hipHostFree(p); }
};

template <typename T> using DevBuf = Owned<T, DeviceMem>;      // grown with reserve(): the mapper's and the engine's per-batch state
template <typename T> using PinnedBuf = Owned<T, PinnedMem>;
template <typename T> using Buf = Owned<T, DeviceMem>;         // alloc() / grow(): the run-long side outputs and the sorter

}  // namespace ngm
