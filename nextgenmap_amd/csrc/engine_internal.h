// engine_internal.h -- private to the library: context layout shared by the C-ABI TU (ngm_hip.cpp) and
// the mapping pipeline (mapper.cpp), plus the entry points that run the DP kernels on an already packed batch.
#pragma once

#include <algorithm>

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ngm_hip.h"
#include "sw_device.h"
#include "affine_device.h"
#include "cigar_device.h"
#include "jit.h"
#include "device_mem.h"

struct ngm_hip_ctx {
	int device = 0;
	ngm_hip_params prm{};
	ngm::SwConst K{};
	ngm::AffConst KA{};
	const ngm::JitKernels *jit = nullptr;  // run-time compiled DP kernels when the corridor has no ahead-of-time build
	int q = 0, c = 0, rl = 0, RW = 0, FW = 0;
	int max_batch = 0;
	hipStream_t stream = nullptr;
	// HBM workspace
	ngm::DevBuf<uint32_t> packed;
	ngm::DevBuf<uint16_t> lens, blk_rows;
	ngm::DevBuf<uint8_t> d_ref, d_qry, d_pair_dir;   // d_pair_dir: the `dir` bytes of the host-pointer entry points (alt_scoring)
	const uint8_t *pair_dir = nullptr;               // ... what the next pack reads: a device array of n bytes, or null (all 0)
	ngm::DevBuf<float> d_scores;
	ngm::DevBuf<uint32_t> dirs;
	ngm::DevBuf<int32_t> d_records;
	ngm::DevBuf<uint16_t> d_runs;
	// pinned staging for the host-pointer entry points
	ngm::PinnedBuf<uint8_t> h_ref, h_qry;
	ngm::PinnedBuf<float> h_scores;
	ngm::PinnedBuf<int32_t> h_records;
	ngm::PinnedBuf<uint16_t> h_runs;
	// profiling
	bool profiling = false;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	bool ev_valid[3] = {false, false, false};
	bool trace_nibbles = false;   // the affine trace matrix in `dirs` holds the 4-bit trace of the packed DP kernel
	std::string error;
};

namespace ngm {
// workspace for n pairs (packed batch, lens, blk_rows); returns 0 or a negative error
int engine_reserve(ngm_hip_ctx *ctx, int n);
// the host-pointer entry points' way into that workspace: the `dir` bytes of n pairs staged for the next pack (null: all pairs use the
// FWD table), and pack_pairs_kernel over n flat rows of q + c window bytes / q read bytes in device memory
int engine_stage_dirs(ngm_hip_ctx *ctx, int n, const char *dir);
int engine_pack(ngm_hip_ctx *ctx, int n, const void *d_ref, const void *d_qry, hipStream_t st);
// DP over ctx->packed / ctx->lens / ctx->blk_rows (filled by pack_pairs_kernel or gather_pairs_kernel)
int engine_score_packed(ngm_hip_ctx *ctx, int mode, int n, float *d_scores, hipStream_t st);
// fin (affine personality only): behind the DP, affine_finish_kernel builds the strings from the trace matrix in one launch instead of the
// traceback into d_runs; d_records keeps the DP's end cells, so engine_affine_traceback_packed can still be run on the batch
struct AlignFinish {
	CigarDevOut *out;                // n entries
	char *bytes;                     // the compact byte stream and its capacity
	unsigned long long capacity;
	unsigned long long *counters;    // [0] stream cursor, [1] alignments left to the host; zeroed by the caller
};
int engine_align_packed(ngm_hip_ctx *ctx, int mode, int n, int32_t *d_records, uint16_t *d_runs, int run_stride, hipStream_t st, const AlignFinish *fin = nullptr);
// the runs of the batch engine_align_packed(..., fin) has just run the DP on (trace matrix and end cells still in place)
int engine_affine_traceback_packed(ngm_hip_ctx *ctx, int n, int32_t *d_records, uint16_t *d_runs, int run_stride, hipStream_t st);
}  // namespace ngm
