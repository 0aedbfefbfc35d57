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
  uint64_t packed = 0;
  const int rc = check_decode_args("seld_grid_decode_tta", logits, is_bf16, w0, nw, W, total, meta_first, meta_len, q0, nq,
                                   Patterns::kOneOrMore, patterns, n_patterns, &packed, K, false, nullptr, det_cell,
                                   det_score, det_count, nullptr, probs_out);
  if (rc != kOk || nq == 0) return rc;
  return launch_meta_frames(is_bf16 ? tta_decode_kernel<true> : tta_decode_kernel<false>, nq, stream_,
                            static_cast<const uint4*>(logits), static_cast<long>(w0), static_cast<long>(nw),
                            static_cast<long>(W), static_cast<long>(total), meta_first, meta_len, static_cast<long>(q0),
                            packed, n_patterns, threshold, K, det_cell, det_score, det_count, probs_out);
}

}  // extern "C"
