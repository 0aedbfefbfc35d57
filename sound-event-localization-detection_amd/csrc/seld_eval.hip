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

// One workgroup per meta-frame q0 + blockIdx.x (the body, shared with seld_tta.hip: seld_eval_core.h).
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
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_grid_decode: K must be in 1..8");
  if (is_bf16 != 0 && is_bf16 != 1) return fail(kErrInvalidArgument, "seld_grid_decode: is_bf16 must be 0 or 1");
  if (total < 1 || W != (total + eval::kHop - 1) / eval::kHop)
    return fail(kErrInvalidArgument, "seld_grid_decode: W must be ceil(total / 50) for a timeline of total >= 1 frames");
  if (w0 < 0 || nw < 1 || w0 + nw > W || q0 < 0 || nq < 0)
    return fail(kErrInvalidArgument, "seld_grid_decode: bad window or meta-frame range");
  if (nq == 0) return kOk;
  if (!logits || !meta_first || !meta_len || !det_cell || !det_score || !det_count)
    return fail(kErrInvalidArgument, "seld_grid_decode: null pointer");
  if ((reinterpret_cast<uintptr_t>(logits) & 15u) != 0 || (probs_out && (reinterpret_cast<uintptr_t>(probs_out) & 15u) != 0))
    return fail(kErrUnsupported, "seld_grid_decode: logits and probs_out must be 16-byte aligned");
  if (nq > 0x7fffffffLL) return fail(kErrUnsupported, "seld_grid_decode: too many meta-frames for one launch");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const auto* src = static_cast<const uint4*>(logits);
  if (is_bf16)
    hipLaunchKernelGGL(grid_decode_kernel<true>, dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, stream, src,
                       static_cast<long>(w0), static_cast<long>(nw), static_cast<long>(W), static_cast<long>(total),
                       meta_first, meta_len, static_cast<long>(q0), threshold, K, det_cell, det_score, det_count,
                       probs_out);
  else
    hipLaunchKernelGGL(grid_decode_kernel<false>, dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, stream, src,
                       static_cast<long>(w0), static_cast<long>(nw), static_cast<long>(W), static_cast<long>(total),
                       meta_first, meta_len, static_cast<long>(q0), threshold, K, det_cell, det_score, det_count,
                       probs_out);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_doa_match(const int32_t* det_cell, const int32_t* det_count, int K, const int32_t* ref_offsets,
                   const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg, int32_t* stats, double* cost,
                   void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_doa_match: K must be in 1..8");
  if (nq < 0 || I < 1 || J < 1) return fail(kErrInvalidArgument, "seld_doa_match: bad extents");
  if (nq == 0) return kOk;
  if (!det_cell || !det_count || !ref_offsets || !stats || !cost)
    return fail(kErrInvalidArgument, "seld_doa_match: null pointer");
  const long n_qc = static_cast<long>(nq) * kC;
  const long blocks = (n_qc + kMatchThreads - 1) / kMatchThreads;
  if (blocks > 0x7fffffffL) return fail(kErrUnsupported, "seld_doa_match: too many meta-frames for one launch");
  hipLaunchKernelGGL(doa_match_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kMatchThreads), 0,
                     static_cast<hipStream_t>(stream_), det_cell, det_count, K, ref_offsets, ref_dirs, n_qc, I, J,
                     thr_deg, stats, cost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
