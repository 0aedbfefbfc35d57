// Threshold sweep of the SELD evaluation on gfx950: every operating point from ONE decode.
//
// No reference counterpart; the definitions are this project's (section 17.1).  The kept detections of a (meta-frame, class)
// are sorted by (score descending, cell ascending) and a cell's peak test does not depend on the threshold, so the list at
// any threshold t >= t0 is a prefix of the list decoded at t0.
//   seld_doa_match_prefix  seld_doa_match / seld_doa_match_dirs for every prefix of every (q, c) in one launch
//                          (seld_match_core.h: match_prefix_entry, next to match_entry): tp and cost per prefix length.
//   seld_sweep_score       per threshold the prefix length of every (q, c), a gather from those tables and the sums
//                          seld_eval.score forms, per chunk of consecutive meta-frames: one lane per threshold, a wave per
//                          chunk, so a meta-frame's 13 classes (S, D, I) stay in one lane.
// Both: no scratch, no atomics, plain stores in a fixed order.
#include "seld_eval_core.h"
#include "seld_match_core.h"

namespace seld {
namespace eval {

constexpr int kMaxThresholds = 64;                    // one lane each

struct Thresholds {
  float t[kMaxThresholds];
};

template <bool kDirs>
__global__ __launch_bounds__(kMatchThreads) void doa_match_prefix_kernel(
    const int32_t* __restrict__ det_cell, const float* __restrict__ det_dir, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs, long n_qc, int I, int J,
    double thr_deg, int32_t* __restrict__ ptp, double* __restrict__ pcost) {
  match_prefix_entry<kDirs>(det_cell, reinterpret_cast<const float2*>(det_dir), det_count, K, ref_offsets, ref_dirs, n_qc,
                            I, J, thr_deg, ptp, pcost);
}

// Workgroup = one wave = chunk blockIdx.x (meta-frames [chunk * blockIdx.x, ...)); lane = threshold.  Every lane walks the
// chunk's (q, c) in order -- the loads are the same address in every lane -- and keeps the per-class sums in registers.
__global__ __launch_bounds__(kMaxThresholds) void sweep_score_kernel(
    const int32_t* __restrict__ ptp, const double* __restrict__ pcost, const float* __restrict__ det_score,
    const int32_t* __restrict__ det_count, int K, const int32_t* __restrict__ ref_offsets, long nq, Thresholds thr, int T,
    long chunk, long n_chunks, int64_t* __restrict__ counts, int64_t* __restrict__ sdi, double* __restrict__ cost) {
  const int lane = threadIdx.x;
  if (lane >= T) return;                                          // (no barriers below)
  const float t = thr.t[lane];
  const long q_lo = static_cast<long>(blockIdx.x) * chunk;
  const long q_hi = q_lo + chunk < nq ? q_lo + chunk : nq;
  int64_t tp_c[kC], fp_c[kC], fn_c[kC], n_c[kC], k_c[kC];
  double cost_c[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    tp_c[c] = fp_c[c] = fn_c[c] = n_c[c] = k_c[c] = 0;
    cost_c[c] = 0.0;
  }
  int64_t s_sum = 0, d_sum = 0, i_sum = 0;
  for (long q = q_lo; q < q_hi; ++q) {
    int64_t fn_q = 0, fp_q = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
      const long qc = q * kC + c;
      const int r = ref_offsets[qc + 1] - ref_offsets[qc];
      int n = det_count[qc];
      n = n < 0 ? 0 : (n > K ? K : n);
      int p = 0;                                                  // leading detections with score >= t (fp32, as the decode)
      bool open = true;
      for (int j = 0; j < n; ++j) {
        open = open && det_score[qc * K + j] >= t;
        p += open ? 1 : 0;
      }
      int tp = ptp[qc * (K + 1) + p];
      int k = r < p ? r : p;
      if (tp < 0) k = tp = -1;                                    // a refused entry, as seld_doa_match reports it
      tp_c[c] += tp;
      fp_c[c] += p - tp;
      fn_c[c] += r - tp;
      n_c[c] += r;
      k_c[c] += k;
      cost_c[c] += pcost[qc * (K + 1) + p];
      fn_q += r - tp;
      fp_q += p - tp;
    }
    s_sum += fn_q < fp_q ? fn_q : fp_q;
    d_sum += fn_q > fp_q ? fn_q - fp_q : 0;
    i_sum += fp_q > fn_q ? fp_q - fn_q : 0;
  }
  const long row = static_cast<long>(lane) * n_chunks + blockIdx.x;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    int64_t* o = counts + (row * kC + c) * 5;
    o[0] = tp_c[c];
    o[1] = fp_c[c];
    o[2] = fn_c[c];
    o[3] = n_c[c];
    o[4] = k_c[c];
    cost[row * kC + c] = cost_c[c];
  }
  sdi[row * 3 + 0] = s_sum;
  sdi[row * 3 + 1] = d_sum;
  sdi[row * 3 + 2] = i_sum;
}

}  // namespace eval
}  // namespace seld

extern "C" {

int seld_doa_match_prefix(const int32_t* det_cell, const float* det_dir, const int32_t* det_count, int K,
                          const int32_t* ref_offsets, const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg,
                          int32_t* ptp, double* pcost, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  long n_qc = 0;
  unsigned blocks = 0;
  const int rc = check_match_args("seld_doa_match_prefix", det_cell, det_dir, K, nq, I, J, true,
                                  {det_count, ref_offsets, ptp, pcost}, false, &n_qc, &blocks);
  if (rc != kOk || nq == 0) return rc;
  hipLaunchKernelGGL(det_dir ? doa_match_prefix_kernel<true> : doa_match_prefix_kernel<false>, dim3(blocks),
                     dim3(kMatchThreads), 0, static_cast<hipStream_t>(stream_), det_cell, det_dir, det_count, K,
                     ref_offsets, ref_dirs, n_qc, det_dir ? 1 : I, det_dir ? 1 : J, thr_deg, ptp, pcost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_sweep_score(const int32_t* ptp, const double* pcost, const float* det_score, const int32_t* det_count, int K,
                     const int32_t* ref_offsets, int64_t nq, const float* thresholds, int T, int64_t chunk,
                     int64_t* counts, int64_t* sdi, double* cost, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_sweep_score: K must be in 1..8");
  if (T < 1 || T > kMaxThresholds) return fail(kErrInvalidArgument, "seld_sweep_score: T must be in 1..64");
  if (!thresholds) return fail(kErrInvalidArgument, "seld_sweep_score: null thresholds");
  Thresholds thr = {};
  for (int i = 0; i < T; ++i) {
    const float v = thresholds[i];
    if (!(v > 0.0f && v <= 1.0f)) return fail(kErrInvalidArgument, "seld_sweep_score: thresholds must lie in (0, 1]");
    if (i && !(v > thresholds[i - 1]))
      return fail(kErrInvalidArgument, "seld_sweep_score: thresholds must be strictly ascending");
    thr.t[i] = v;
  }
  if (nq < 0 || chunk < 1) return fail(kErrInvalidArgument, "seld_sweep_score: bad extents");
  if (nq == 0) return kOk;
  if (!ptp || !pcost || !det_score || !det_count || !ref_offsets || !counts || !sdi || !cost)
    return fail(kErrInvalidArgument, "seld_sweep_score: null pointer");
  const long n_chunks = static_cast<long>((nq + chunk - 1) / chunk);
  if (n_chunks > 0x7fffffffL) return fail(kErrUnsupported, "seld_sweep_score: too many chunks for one launch");
  hipLaunchKernelGGL(sweep_score_kernel, dim3(static_cast<unsigned>(n_chunks)), dim3(kMaxThresholds), 0,
                     static_cast<hipStream_t>(stream_), ptp, pcost, det_score, det_count, K, ref_offsets,
                     static_cast<long>(nq), thr, T, static_cast<long>(chunk), n_chunks, counts, sdi, cost);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
