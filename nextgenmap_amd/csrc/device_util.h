// device_util.h -- what the host sides of the run-long side outputs (bam_sort.cpp, and through side_output.h coverage.cpp, snp.cpp and
// count.cpp) share: device memory that frees itself and takes a host vector, a guard for the calling thread's device, the launch grid of
// the 256-thread kernels, and the HIP error check of the C ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "device_mem.h"   // ngm::Buf
#include "refindex.h"   // ngm::pipeline_set_error

// a failed HIP call: its text becomes ngm_pipeline_last_error() and the calling function returns -5
#define NGM_HIP_TRY(expr)                                                                       \
	do {                                                                                        \
		hipError_t e_ = (expr);                                                                 \
		if (e_ != hipSuccess) {                                                                 \
			ngm::pipeline_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return -5;                                                                          \
		}                                                                                       \
	} while (0)

namespace ngm {

// a host vector into a buffer of exactly its size (true: placed; the copy is through once st is synchronised)
template <typename T> bool put(Buf<T> &b, const std::vector<T> &v, hipStream_t st) {
	return !b.alloc(v.size()) && (v.empty() || hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st) == hipSuccess);
}

struct DeviceGuard {   // a call from a thread that works on another GPU leaves that thread's device as it was
	int prev = -1;
	explicit DeviceGuard(int device) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != device) (void) hipSetDevice(device); else prev = -1; }
	~DeviceGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
};

inline unsigned blocks_of(uint64_t n) { return (unsigned) ((n + 255) / 256); }

}  // namespace ngm
