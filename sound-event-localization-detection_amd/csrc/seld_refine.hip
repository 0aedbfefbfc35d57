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

template <bool kBf16, bool kTta, class... Args>
void launch_refine(long nq, hipStream_t stream, Args... args) {
  hipLaunchKernelGGL((refine_decode_kernel<kBf16, kTta>), dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, stream,
                     args...);
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
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_grid_decode_refine: K must be in 1..8");
  if (is_bf16 != 0 && is_bf16 != 1) return fail(kErrInvalidArgument, "seld_grid_decode_refine: is_bf16 must be 0 or 1");
  if (n_patterns < 0 || n_patterns > kMaxPatterns)
    return fail(kErrInvalidArgument, "seld_grid_decode_refine: n_patterns must be 0 (the plain walk) or in 1..16");
  if ((n_patterns == 0) != (patterns == nullptr))
    return fail(kErrInvalidArgument, "seld_grid_decode_refine: patterns must be NULL exactly when n_patterns is 0");
  uint64_t packed = 0;
  unsigned seen = 0;
  for (int n = 0; n < n_patterns; ++n) {
    const int32_t p = patterns[n];
    if (p < 0 || p >= kMaxPatterns) return fail(kErrInvalidArgument, "seld_grid_decode_refine: pattern outside 0..15");
    if (seen & (1u << p)) return fail(kErrInvalidArgument, "seld_grid_decode_refine: duplicate pattern");
    seen |= 1u << p;
    packed |= static_cast<uint64_t>(p) << (4 * n);
  }
  if (total < 1 || W != (total + eval::kHop - 1) / eval::kHop)
    return fail(kErrInvalidArgument,
                "seld_grid_decode_refine: W must be ceil(total / 50) for a timeline of total >= 1 frames");
  if (w0 < 0 || nw < 1 || w0 + nw > W || q0 < 0 || nq < 0)
    return fail(kErrInvalidArgument, "seld_grid_decode_refine: bad window or meta-frame range");
  if (!cell_unit || !det_dir) return fail(kErrInvalidArgument, "seld_grid_decode_refine: null cell_unit or det_dir");
  if (nq == 0) return kOk;
  if (!logits || !meta_first || !meta_len || !det_cell || !det_score || !det_count)
    return fail(kErrInvalidArgument, "seld_grid_decode_refine: null pointer");
  if ((reinterpret_cast<uintptr_t>(logits) & 15u) != 0 || (reinterpret_cast<uintptr_t>(det_dir) & 15u) != 0 ||
      (probs_out && (reinterpret_cast<uintptr_t>(probs_out) & 15u) != 0))
    return fail(kErrUnsupported, "seld_grid_decode_refine: logits, det_dir and probs_out must be 16-byte aligned");
  if (nq > 0x7fffffffLL) return fail(kErrUnsupported, "seld_grid_decode_refine: too many meta-frames for one launch");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const auto* src = static_cast<const uint4*>(logits);
  const long lw0 = static_cast<long>(w0), lnw = static_cast<long>(nw), lW = static_cast<long>(W);
  const long ltotal = static_cast<long>(total), lq0 = static_cast<long>(q0), lnq = static_cast<long>(nq);
  const int n_pat = n_patterns ? n_patterns : 1;
#define SELD_REFINE_LAUNCH(BF16, TTA)                                                                                    \
  launch_refine<BF16, TTA>(lnq, stream, src, lw0, lnw, lW, ltotal, meta_first, meta_len, lq0, packed, n_pat, threshold, \
                           K, cell_unit, det_cell, det_score, det_count, det_dir, probs_out)
  if (n_patterns) {
    if (is_bf16) SELD_REFINE_LAUNCH(true, true); else SELD_REFINE_LAUNCH(false, true);
  } else {
    if (is_bf16) SELD_REFINE_LAUNCH(true, false); else SELD_REFINE_LAUNCH(false, false);
  }
#undef SELD_REFINE_LAUNCH
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_doa_match_dirs(const float* det_dir, const int32_t* det_count, int K, const int32_t* ref_offsets,
                        const int32_t* ref_dirs, int64_t nq, double thr_deg, int32_t* stats, double* cost,
                        void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_doa_match_dirs: K must be in 1..8");
  if (nq < 0) return fail(kErrInvalidArgument, "seld_doa_match_dirs: bad extents");
  if (nq == 0) return kOk;
  if (!det_dir || !det_count || !ref_offsets || !stats || !cost)
    return fail(kErrInvalidArgument, "seld_doa_match_dirs: null pointer");
  if ((reinterpret_cast<uintptr_t>(det_dir) & 7u) != 0)
    return fail(kErrUnsupported, "seld_doa_match_dirs: det_dir must be 8-byte aligned");
  const long n_qc = static_cast<long>(nq) * kC;
  const long blocks = (n_qc + kMatchThreads - 1) / kMatchThreads;
  if (blocks > 0x7fffffffL) return fail(kErrUnsupported, "seld_doa_match_dirs: too many meta-frames for one launch");
  hipLaunchKernelGGL(doa_match_dirs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kMatchThreads), 0,
                     static_cast<hipStream_t>(stream_), det_dir, det_count, K, ref_offsets, ref_dirs, n_qc, thr_deg, stats,
                     cost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
