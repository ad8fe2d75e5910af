// ctd_internal.h -- what one csrc/*.hip file calls in another: nothing here has a single-file caller.  (The C entry
// points of include/ctd_hip.h live with their kernels; predicates that several of them share are in ctd_validate.h.)
#pragma once
#include "ctd_common.h"

namespace ctd {

// kernel timing hooks (ctd_api.hip)
void timing_begin(hipStream_t stream);          // records the start event of the dominant kernel
void timing_end(hipStream_t stream, int columns);

// ncc_exact.hip (called by the NCC entry points in ncc_fast.hip)
size_t ncc_exact_workspace_bytes(int frames, int C, int H, int W, int D, int bs, bool per_frame_pattern);
int ncc_exact_f32(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H,
                  int W, int D, int bs, void* workspace, size_t workspace_bytes, hipStream_t stream);
int ncc_exact_argmax_f32(const float* in0, const float* in1, long in1_frame_stride, float* vol_out, int64_t* idx,
                         float* best, int frames, int H, int W, int D, int bs, void* workspace,
                         size_t workspace_bytes, hipStream_t stream);

// ncc_fast.hip: buffers of the in-kernel ranking (all inside the caller's workspace, laid out by ncc_fast_f32); shared
// with the all-D kernel (ncc_alld.hip), the ranked fix-up (ncc_fixup.hip) and the tail kernel (argmax_rerank.hip)
struct RankPlan {
  float eps;                  // in: re-ranking margin requested by the caller
  int64_t* idx;               // in: [frames][H][W] indices (written by the all-D kernel, corrected by the resolve pass)
  float* best;                // in: [frames][H][W] best scores, or null (out: best_scratch then)
  unsigned char* flags;       // [frames][H][W] 1 = pixel is on the work list (written by the all-D kernel)
  WorkList work;              // work list of the pixels the exact re-scoring has to settle (counters cleared by the
                              // pre-pass kernel)
  float* best_scratch;        // [frames][H][W] best score when the caller does not ask for it
  // what the tail kernel (runs | decode | resolve roles, argmax_rerank.hip) needs of the volume pass's workspace
  const float* run_vals;      // [frames][H][D] exact values of the listed fully clamped runs
  const unsigned long long* run_rows;
  unsigned* counters;         // [0] listed frame windows (the tail kernel clears it), [1] listed pattern windows, [2] listed run
                              // rows, [3] copy of [0] made by the ranked fix-up kernel for the tail kernel
  const unsigned long long *flag_a, *flag_b;   // lists of the listed frame / pattern windows
  const float* v1;            // pattern reciprocal-deviation planes (0 = listed window), row pitch W1, column x at x + xoff
  int W1, xoff;
  size_t bytes;               // workspace bytes up to the end of these buffers
};

// costvol_sep.hip: separable block SAD / MSE cost volume through the all-D pipeline (block 9, W % 4 == 0); workspace = padded operand planes
bool costvol_sep_supported(int H, int W, int D, int bs, int type);
size_t costvol_sep_workspace_bytes(int frames, int H, int W, int D, bool per_frame_pattern);
int costvol_sep_f32(const float* im, const float* pat, long pat_frame_stride, float* cost, int frames, int H, int W, int D,
                    int type, void* workspace, size_t workspace_bytes, hipStream_t stream);

// argmax_rerank.hip
int argmax_rerank_f32(const float* vol, const float* in0, const float* in1, long in1_frame_stride, int64_t* idx,
                      float* best, int frames, int D, int H, int W, int bs, float eps, void* workspace,
                      size_t workspace_bytes, bool counter_cleared, hipStream_t stream);
int rank_tail_f32(const RankPlan& rp, float* vol, const float* in0, const float* in1, long in1_frame_stride,
                  int64_t* idx, float* best, int frames, int D, int H, int W, int bs, hipStream_t stream);

// ncc_alld.hip: compute units of the current device (cached)
int device_cu_count();

// costvol_fast.hip: ranking instantiations of the volume kernels (Top2Planes: ctd_top2.h), for costvol_argmin.hip
struct Top2Planes;
bool costvol_rank_supported(int frames, int H, int W, int D, int bs);
int costvol_rank_f32(const float* im, const float* pat, long pat_frame_stride, const Top2Planes& top, int frames, int H,
                     int W, int D, int bs, int type, float eps, hipStream_t stream);

}  // namespace ctd
