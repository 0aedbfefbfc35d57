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
constexpr int kMatchThreads = 16;                      // one lane per (q, c); 40 KB of LDS per workgroup
constexpr int kMaxSide = 8;

// Great-circle angle in degrees, float64, from the unit vectors (atan2 of |u x v| and u . v: accurate at 0 and 180
// degrees).  Identical directions are exactly 0.
__device__ __forceinline__ double angle_deg(double az1, double el1, double az2, double el2) {
  if (az1 == az2 && el1 == el2) return 0.0;
  constexpr double kRad = 3.141592653589793 / 180.0;
  const double a1 = az1 * kRad, e1 = el1 * kRad, a2 = az2 * kRad, e2 = el2 * kRad;
  const double x1 = cos(e1) * cos(a1), y1 = cos(e1) * sin(a1), z1 = sin(e1);
  const double x2 = cos(e2) * cos(a2), y2 = cos(e2) * sin(a2), z2 = sin(e2);
  const double cx = y1 * z2 - z1 * y2, cy = z1 * x2 - x1 * z2, cz = x1 * y2 - y1 * x2;
  const double dot = x1 * x2 + y1 * y2 + z1 * z2;
  return atan2(sqrt(cx * cx + cy * cy + cz * cz), dot) * (180.0 / 3.141592653589793);
}

__global__ __launch_bounds__(kMatchThreads) void doa_match_kernel(
    const int32_t* __restrict__ det_cell, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs, long n_qc, int I, int J,
    double thr_deg, int32_t* __restrict__ stats, double* __restrict__ cost) {
  __shared__ double dist[kMaxSide * kMaxSide][kMatchThreads];    // [row][col], lane-minor: no bank conflicts
  __shared__ double dp[1 << kMaxSide][kMatchThreads];            // minimum cost per set of used columns
  const int lane = threadIdx.x;
  const long qc = static_cast<long>(blockIdx.x) * kMatchThreads + lane;
  if (qc >= n_qc) return;                                         // (no barriers below)
  const int r0 = ref_offsets[qc];
  const int nr = ref_offsets[qc + 1] - r0;
  const int np = det_count[qc];
  int32_t* st = stats + qc * 4;
  if (nr < 0 || nr > kMaxSide || np < 0 || np > K) {             // refused by the host; never read out of range
    st[0] = nr;
    st[1] = np;
    st[2] = -1;
    st[3] = -1;
    cost[qc] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  // rows = the smaller side, so that an injection of size k = rows covers every row
  const bool refs_are_rows = nr <= np;
  const int rows = refs_are_rows ? nr : np, cols = refs_are_rows ? np : nr;
  uint64_t adj = 0;                                               // bit 8 r + p: reference r within thr of detection p
  const double cell_az = 360.0 / J, cell_el = 180.0 / I;
  for (int r = 0; r < nr; ++r) {
    const double raz = ref_dirs[2 * (r0 + r)], rel = ref_dirs[2 * (r0 + r) + 1];
    for (int p = 0; p < np; ++p) {
      const int cell = det_cell[qc * K + p];
      const int ci = cell / J, cj = cell - ci * J;
      const double d = angle_deg(raz, rel, -180.0 + (cj + 0.5) * cell_az, -90.0 + (ci + 0.5) * cell_el);
      if (d <= thr_deg) adj |= 1ull << (8 * r + p);
      dist[refs_are_rows ? r * kMaxSide + p : p * kMaxSide + r][lane] = d;
    }
  }
  // tp = maximum matching within the threshold = min over reference sets S of (nr - |S| + |N(S)|) (Hall / Koenig)
  int tp = nr < np ? nr : np;
  for (uint32_t s = 1; s < (1u << nr); ++s) {
    uint32_t nb = 0;
    for (int r = 0; r < nr; ++r)
      if ((s >> r) & 1u) nb |= static_cast<uint32_t>(adj >> (8 * r)) & 0xffu;
    const int v = nr - __popc(s) + __popc(nb);
    tp = v < tp ? v : tp;
  }
  // cost = minimum total distance of an injection rows -> cols: dp over the used columns, row r = popcount - 1
  const int k = rows;
  double best = 0.0;
  if (k > 0) {
    best = __longlong_as_double(0x7ff0000000000000LL);         // +inf
    dp[0][lane] = 0.0;
    for (uint32_t mask = 1; mask < (1u << cols); ++mask) {
      const int pc = __popc(mask);
      if (pc > k) continue;
      const int r = pc - 1;
      double v = __longlong_as_double(0x7ff0000000000000LL);
      for (int b = 0; b < cols; ++b) {
        if (!((mask >> b) & 1u)) continue;
        const double cand = dp[mask ^ (1u << b)][lane] + dist[r * kMaxSide + b][lane];
        v = cand < v ? cand : v;
      }
      dp[mask][lane] = v;
      if (pc == k) best = v < best ? v : best;
    }
  }
  st[0] = nr;
  st[1] = np;
  st[2] = k;
  st[3] = tp;
  cost[qc] = best;
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
