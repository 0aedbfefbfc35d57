// Test-time augmentation of the SELD decode on gfx950: the grid maps of up to 16 transformed copies
// of every window -- the sign-and-swap transforms of the FOA channels, section 11.1 -- averaged in the ORIGINAL frame
// before the peak test.
//
//   seld_grid_decode_tta  logits [n][nw][250][648][14]: stack n holds the windows gathered with pattern p_n.  The decode
//                         of seld_grid_decode (seld_eval_core.h) with one more inner loop level: a meta-frame's rows are
//                         walked in (frame, window, n) ascending order, the thread that owns cell x reads the staged row
//                         at cell_dest(p_n)[x] -- three integer selects on the pattern's bits, no table and no extra
//                         memory traffic -- and a frame's sum is divided once by n_w * n.  With patterns = (0) that is
//                         the plain decode's order and arithmetic: bit-identical outputs.
// The patterns travel by value in the kernel arguments (16 x 4 bits), so the launch needs no upload and stays
// graph-capturable.
#include "seld_eval_core.h"

namespace seld {
namespace eval {

template <bool kBf16>
__global__ __launch_bounds__(kThreads) void tta_decode_kernel(
    const uint4* __restrict__ logits, long w0, long nw, long W, long total, const int64_t* __restrict__ meta_first,
    const int32_t* __restrict__ meta_len, long q0, uint64_t patterns, int n_pat, float threshold, int K,
    int32_t* __restrict__ det_cell, float* __restrict__ det_score, int32_t* __restrict__ det_count,
    float* __restrict__ probs_out) {
  decode_meta_frame<kBf16, true>(logits, w0, nw, W, total, meta_first, meta_len, q0, threshold, K, det_cell, det_score,
                                 det_count, probs_out, patterns, n_pat, nw * kWin * static_cast<long>(Row<kBf16>::kChunks));
}

}  // namespace eval
}  // namespace seld

extern "C" {

int seld_grid_decode_tta(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                         const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq,
                         const int32_t* patterns, int n_patterns, float threshold, int K, int32_t* det_cell,
                         float* det_score, int32_t* det_count, float* probs_out, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_grid_decode_tta: K must be in 1..8");
  if (is_bf16 != 0 && is_bf16 != 1) return fail(kErrInvalidArgument, "seld_grid_decode_tta: is_bf16 must be 0 or 1");
  if (n_patterns < 1 || n_patterns > kMaxPatterns)
    return fail(kErrInvalidArgument, "seld_grid_decode_tta: n_patterns must be in 1..16");
  if (!patterns) return fail(kErrInvalidArgument, "seld_grid_decode_tta: null pointer");
  uint64_t packed = 0;
  unsigned seen = 0;
  for (int n = 0; n < n_patterns; ++n) {
    const int32_t p = patterns[n];
    if (p < 0 || p >= kMaxPatterns) return fail(kErrInvalidArgument, "seld_grid_decode_tta: pattern outside 0..15");
    if (seen & (1u << p)) return fail(kErrInvalidArgument, "seld_grid_decode_tta: duplicate pattern");
    seen |= 1u << p;
    packed |= static_cast<uint64_t>(p) << (4 * n);
  }
  if (total < 1 || W != (total + eval::kHop - 1) / eval::kHop)
    return fail(kErrInvalidArgument, "seld_grid_decode_tta: W must be ceil(total / 50) for a timeline of total >= 1 frames");
  if (w0 < 0 || nw < 1 || w0 + nw > W || q0 < 0 || nq < 0)
    return fail(kErrInvalidArgument, "seld_grid_decode_tta: bad window or meta-frame range");
  if (nq == 0) return kOk;
  if (!logits || !meta_first || !meta_len || !det_cell || !det_score || !det_count)
    return fail(kErrInvalidArgument, "seld_grid_decode_tta: null pointer");
  if ((reinterpret_cast<uintptr_t>(logits) & 15u) != 0 || (probs_out && (reinterpret_cast<uintptr_t>(probs_out) & 15u) != 0))
    return fail(kErrUnsupported, "seld_grid_decode_tta: logits and probs_out must be 16-byte aligned");
  if (nq > 0x7fffffffLL) return fail(kErrUnsupported, "seld_grid_decode_tta: too many meta-frames for one launch");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const auto* src = static_cast<const uint4*>(logits);
  if (is_bf16)
    hipLaunchKernelGGL(tta_decode_kernel<true>, dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, stream, src,
                       static_cast<long>(w0), static_cast<long>(nw), static_cast<long>(W), static_cast<long>(total),
                       meta_first, meta_len, static_cast<long>(q0), packed, n_patterns, threshold, K, det_cell, det_score,
                       det_count, probs_out);
  else
    hipLaunchKernelGGL(tta_decode_kernel<false>, dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, stream, src,
                       static_cast<long>(w0), static_cast<long>(nw), static_cast<long>(W), static_cast<long>(total),
                       meta_first, meta_len, static_cast<long>(q0), packed, n_patterns, threshold, K, det_cell, det_score,
                       det_count, probs_out);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
