// Sub-cell DOA refinement of the SELD decode on gfx950: every detection gets a direction finer than
// its 10-degree cell, from the class map the decode already holds in LDS.
//
// No reference counterpart; the definitions are this project's (section 15.1).
//   seld_grid_decode_refine  the decode of seld_grid_decode / seld_grid_decode_tta (seld_eval_core.h, the same body) with an
//                            epilogue after a class's top-K selection: lane r of the wave that selected the class sums
//                            P_q[y][c] u(y) over detection r's peak cell and its up-to-8 neighbours -- nine LDS reads, the
//                            unit vectors u from a 7.8 KB table the host built -- and writes (az, el) of the sum.  No extra
//                            pass over HBM and no second launch; cells, scores, counts and P_q are the un-refined
//                            export's bit for bit.
//   seld_doa_match_dirs      seld_doa_match (seld_match_core.h, the same body) on those float directions, widened to
//                            float64, in place of the cell centres.
// Both keep the decode's properties: no scratch, no atomics, plain vector stores, a fixed order.
#include "seld_eval_core.h"
#include "seld_match_core.h"

namespace seld {
namespace eval {

template <bool kBf16, bool kTta>
__global__ __launch_bounds__(kThreads) void refine_decode_kernel(
    const uint4* __restrict__ logits, long w0, long nw, long W, long total, const int64_t* __restrict__ meta_first,
    const int32_t* __restrict__ meta_len, long q0, uint64_t patterns, int n_pat, float threshold, int K,
    const float* __restrict__ cell_unit, int32_t* __restrict__ det_cell, float* __restrict__ det_score,
    int32_t* __restrict__ det_count, float* __restrict__ det_dir, float* __restrict__ probs_out) {
  decode_meta_frame<kBf16, kTta, true>(logits, w0, nw, W, total, meta_first, meta_len, q0, threshold, K, det_cell,
                                       det_score, det_count, probs_out, patterns, n_pat,
                                       kTta ? nw * kWin * static_cast<long>(Row<kBf16>::kChunks) : 0, cell_unit, det_dir);
}

// One lane per (q, c); a detection's direction is what the refined decode wrote.
__global__ __launch_bounds__(kMatchThreads) void doa_match_dirs_kernel(
    const float* __restrict__ det_dir, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs, long n_qc, double thr_deg,
    int32_t* __restrict__ stats, double* __restrict__ cost) {
  match_entry<true>(nullptr, reinterpret_cast<const float2*>(det_dir), det_count, K, ref_offsets, ref_dirs, n_qc, 1, 1,
                    thr_deg, stats, cost);
}

}  // namespace eval
}  // namespace seld

extern "C" {

int seld_grid_decode_refine(const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W, int64_t total,
                            const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq,
                            const int32_t* patterns, int n_patterns, float threshold, int K, const float* cell_unit,
                            int32_t* det_cell, float* det_score, int32_t* det_count, float* det_dir, float* probs_out,
                            void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  uint64_t packed = 0;
  const int rc = check_decode_args("seld_grid_decode_refine", logits, is_bf16, w0, nw, W, total, meta_first, meta_len, q0,
                                   nq, Patterns::kAny, patterns, n_patterns, &packed, K, true, cell_unit, det_cell,
                                   det_score, det_count, det_dir, probs_out);
  if (rc != kOk || nq == 0) return rc;
  const auto kernel = n_patterns ? (is_bf16 ? refine_decode_kernel<true, true> : refine_decode_kernel<false, true>)
                                 : (is_bf16 ? refine_decode_kernel<true, false> : refine_decode_kernel<false, false>);
  return launch_meta_frames(kernel, nq, stream_, static_cast<const uint4*>(logits), static_cast<long>(w0),
                            static_cast<long>(nw), static_cast<long>(W), static_cast<long>(total), meta_first, meta_len,
                            static_cast<long>(q0), packed, n_patterns ? n_patterns : 1, threshold, K, cell_unit, det_cell,
                            det_score, det_count, det_dir, probs_out);
}

int seld_doa_match_dirs(const float* det_dir, const int32_t* det_count, int K, const int32_t* ref_offsets,
                        const int32_t* ref_dirs, int64_t nq, double thr_deg, int32_t* stats, double* cost,
                        void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  long n_qc = 0;
  unsigned blocks = 0;
  const int rc = check_match_args("seld_doa_match_dirs", nullptr, det_dir, K, nq, 1, 1, true,
                                  {det_count, ref_offsets, stats, cost}, false, &n_qc, &blocks);
  if (rc != kOk || nq == 0) return rc;
  hipLaunchKernelGGL(doa_match_dirs_kernel, dim3(blocks), dim3(kMatchThreads), 0, static_cast<hipStream_t>(stream_),
                     det_dir, det_count, K, ref_offsets, ref_dirs, n_qc, thr_deg, stats, cost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
