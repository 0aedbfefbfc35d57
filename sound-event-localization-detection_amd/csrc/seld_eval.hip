// SELD evaluation on gfx950: spatial grid maps -> DOA events, and the location-aware matching behind the metrics.
//
// No reference counterpart (the reference's test_model only reports argmax accuracy per grid cell, trainer.py:394-711);
// the definitions are this project's:
//   seld_grid_decode  softmax of every (window, frame, cell) row of the model's [W][250][648][14] output, averaged over
//                     the overlapping windows (hop 50) and over the frames of each 100 ms meta-frame, then a class-wise
//                     3x3 peak test and a top-K selection per (meta-frame, class).  One streaming pass over the logits.
//   seld_doa_match    per (meta-frame, class): great-circle distances between detections (cell centres) and references,
//                     minimum-cost assignment of size min(R, P) and the maximum-cardinality matching within the DOA
//                     threshold.
// Both are deterministic: fixed summation order, no float atomics.
#include "seld_eval_core.h"
#include "seld_match_core.h"

namespace seld {
namespace eval {

// One workgroup per meta-frame q0 + blockIdx.x (the body, shared with seld_tta.hip and seld_refine.hip: seld_eval_core.h).
template <bool kBf16>
__global__ __launch_bounds__(kThreads) void grid_decode_kernel(
    const uint4* __restrict__ logits, long w0, long nw, long W, long total, const int64_t* __restrict__ meta_first,
    const int32_t* __restrict__ meta_len, long q0, float threshold, int K, int32_t* __restrict__ det_cell,
    float* __restrict__ det_score, int32_t* __restrict__ det_count, float* __restrict__ probs_out) {
  decode_meta_frame<kBf16, false>(logits, w0, nw, W, total, meta_first, meta_len, q0, threshold, K, det_cell,
                                  det_score, det_count, probs_out, 0, 1, 0);
}

// ---- matching ----------------------------------------------------------------------------------------------------
// One lane per (q, c) (the body, shared with seld_refine.hip: seld_match_core.h); a detection's direction is its cell centre.
__global__ __launch_bounds__(kMatchThreads) void doa_match_kernel(
    const int32_t* __restrict__ det_cell, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs, long n_qc, int I, int J,
    double thr_deg, int32_t* __restrict__ stats, double* __restrict__ cost) {
  match_entry<false>(det_cell, nullptr, det_count, K, ref_offsets, ref_dirs, n_qc, I, J, thr_deg, stats, cost);
}

}  // namespace eval
}  // namespace seld

extern "C" {

int seld_grid_decode(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                     const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq, float threshold, int K,
                     int32_t* det_cell, float* det_score, int32_t* det_count, float* probs_out, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  const int rc = check_decode_args("seld_grid_decode", logits, is_bf16, w0, nw, W, total, meta_first, meta_len, q0, nq,
                                   Patterns::kNone, nullptr, 0, nullptr, K, false, nullptr, det_cell, det_score, det_count,
                                   nullptr, probs_out);
  if (rc != kOk || nq == 0) return rc;
  return launch_meta_frames(is_bf16 ? grid_decode_kernel<true> : grid_decode_kernel<false>, nq, stream_,
                            static_cast<const uint4*>(logits), static_cast<long>(w0), static_cast<long>(nw),
                            static_cast<long>(W), static_cast<long>(total), meta_first, meta_len, static_cast<long>(q0),
                            threshold, K, det_cell, det_score, det_count, probs_out);
}

int seld_doa_match(const int32_t* det_cell, const int32_t* det_count, int K, const int32_t* ref_offsets,
                   const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg, int32_t* stats, double* cost,
                   void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  long n_qc = 0;
  unsigned blocks = 0;
  const int rc = check_match_args("seld_doa_match", det_cell, nullptr, K, nq, I, J, true,
                                  {det_count, ref_offsets, stats, cost}, false, &n_qc, &blocks);
  if (rc != kOk || nq == 0) return rc;
  hipLaunchKernelGGL(doa_match_kernel, dim3(blocks), dim3(kMatchThreads), 0, static_cast<hipStream_t>(stream_), det_cell,
                     det_count, K, ref_offsets, ref_dirs, n_qc, I, J, thr_deg, stats, cost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
