// Segment-based, class-macro SELD metrics with jackknife replicates on gfx950.
//
// No reference counterpart; the definitions are this project's (section 18.1), after the DCASE 2022/23 segment-based metric.
//   seld_doa_assign       per (q, c) the minimum-cost assignment ITSELF: match_entry's distances and dp (seld_match_core.h:
//                         fill_distances and min_cost_assignment, shared) plus a one-byte choice table and a backtrack
//   seld_segment_score    two launches: the counts of every (1 s block, class), then the blocks of a recording folded in
//                         ascending order
//   seld_jackknife_score  one lane per leave-one-recording-out replicate: micro and macro F / ER / LE / LR / SELD
// All: no scratch, no atomics, plain stores in a fixed order.
#include "seld_eval_core.h"
#include "seld_match_core.h"

namespace seld {
namespace eval {

constexpr int kBlockFrames = 10;                      // meta-frames per block: 1 s
constexpr int kSegStats = 8;                          // Nref, Npred, TP, FPs, FP, FN, DE_TP, DE_FN
constexpr int kRecCounts = 11;                        // the eight plus S_c, D_c, I_c
constexpr int kFigures = 5;                           // F, ER, LE, LR, SELD
constexpr int kSegThreads = 256;
constexpr int kFoldThreads = 16;                      // 13 class lanes and one for the micro S, D, I
constexpr int kJackThreads = 64;

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// One lane per (q, c) (the body, next to match_entry: seld_match_core.h).
template <bool kDirs>
__global__ __launch_bounds__(kMatchThreads) void doa_assign_kernel(
    const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs, long n_qc, int I, int J,
    double* __restrict__ pair_dist) {
  assign_entry<kDirs>(det_cell, det_dir, det_count, K, ref_offsets, ref_dirs, n_qc, I, J, pair_dist);
}

// Workgroup = recording s; its (block, class) pairs are dealt to the lanes.  Block x of the recording covers meta-frames
// seg_offsets[s] + 10 x .. min(.. + 10, seg_offsets[s + 1]) - 1 and is row block_offsets[s] + x of the outputs.
__global__ __launch_bounds__(kSegThreads) void segment_blocks_kernel(
    const double* __restrict__ pair_dist, const int32_t* __restrict__ det_count, int K,
    const int32_t* __restrict__ ref_offsets, const int64_t* __restrict__ seg_offsets,
    const int64_t* __restrict__ block_offsets, double thr_deg, int32_t* __restrict__ seg_stats, double* __restrict__ seg_de) {
  const long s = blockIdx.x;
  const long q_lo = seg_offsets[s], q_hi = seg_offsets[s + 1];
  const long b_lo = block_offsets[s], n_blocks = block_offsets[s + 1] - b_lo;
  for (long item = threadIdx.x; item < n_blocks * kC; item += kSegThreads) {
    const long x = item / kC;
    const int c = static_cast<int>(item - x * kC);
    const long q0 = q_lo + x * kBlockFrames;
    const long q1 = q0 + kBlockFrames < q_hi ? q0 + kBlockFrames : q_hi;
    double sum[kMaxSide];
    int cnt[kMaxSide];
#pragma unroll
    for (int r = 0; r < kMaxSide; ++r) {
      sum[r] = 0.0;
      cnt[r] = 0;
    }
    int nref = 0, npred = 0;
    for (long q = q0; q < q1; ++q) {
      const long qc = q * kC + c;
      const int rm = ref_offsets[qc + 1] - ref_offsets[qc];
      int pm = det_count[qc];
      pm = pm < 0 ? 0 : (pm > K ? K : pm);
      nref = rm > nref ? rm : nref;
      npred = pm > npred ? pm : npred;
      if (rm > 0 && pm > 0) {                                     // a common frame
#pragma unroll
        for (int r = 0; r < kMaxSide; ++r) {
          const double d = pair_dist[qc * kMaxSide + r];
          if (d == d) {
            sum[r] += d;
            cnt[r] += 1;
          }
        }
      }
    }
    int tp = 0, fps = 0, fp = 0, fn = 0, de_tp = 0, de_fn = 0;
    double de = 0.0;
#pragma unroll
    for (int r = 0; r < kMaxSide; ++r) {
      if (cnt[r] > 0) {
        const double avg = sum[r] / cnt[r];
        de += avg;
        de_tp += 1;
        if (avg <= thr_deg) tp += 1; else fps += 1;
      }
    }
    if (nref > 0 && npred > 0) {
      if (de_tp > 0) {
        fp = npred > nref ? npred - nref : 0;
        fn = nref > npred ? nref - npred : 0;
      } else {                                                    // never active in the same frame
        fn = nref;
        fp = npred;
      }
    } else if (nref > 0) {
      fn = nref;
    } else {
      fp = npred;
    }
    de_fn = fn;
    int32_t* o = seg_stats + ((b_lo + x) * kC + c) * kSegStats;
    o[0] = nref;
    o[1] = npred;
    o[2] = tp;
    o[3] = fps;
    o[4] = fp;
    o[5] = fn;
    o[6] = de_tp;
    o[7] = de_fn;
    seg_de[(b_lo + x) * kC + c] = de;
  }
}

// Workgroup = recording s.  Lane c < 13 folds class c's blocks in ascending order; lane 13 the micro S, D, I.
__global__ __launch_bounds__(kFoldThreads) void segment_fold_kernel(
    const int32_t* __restrict__ seg_stats, const double* __restrict__ seg_de, const int64_t* __restrict__ block_offsets,
    int64_t* __restrict__ rec_counts, int64_t* __restrict__ rec_sdi, double* __restrict__ rec_de) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const long b_lo = block_offsets[s], b_hi = block_offsets[s + 1];
  if (lane < kC) {
    int64_t acc[kRecCounts];
#pragma unroll
    for (int i = 0; i < kRecCounts; ++i) acc[i] = 0;
    double de = 0.0;
    for (long b = b_lo; b < b_hi; ++b) {
      const int32_t* in = seg_stats + (b * kC + lane) * kSegStats;
#pragma unroll
      for (int i = 0; i < kSegStats; ++i) acc[i] += in[i];
      const int64_t loc_fp = static_cast<int64_t>(in[3]) + in[4], loc_fn = in[5];
      acc[8] += loc_fp < loc_fn ? loc_fp : loc_fn;
      acc[9] += loc_fn > loc_fp ? loc_fn - loc_fp : 0;
      acc[10] += loc_fp > loc_fn ? loc_fp - loc_fn : 0;
      de += seg_de[b * kC + lane];
    }
    int64_t* o = rec_counts + (s * kC + lane) * kRecCounts;
#pragma unroll
    for (int i = 0; i < kRecCounts; ++i) o[i] = acc[i];
    rec_de[s * kC + lane] = de;
  } else if (lane == kC) {
    int64_t s_sum = 0, d_sum = 0, i_sum = 0;
    for (long b = b_lo; b < b_hi; ++b) {
      int64_t loc_fp = 0, loc_fn = 0;
#pragma unroll
      for (int c = 0; c < kC; ++c) {
        const int32_t* in = seg_stats + (b * kC + c) * kSegStats;
        loc_fp += static_cast<int64_t>(in[3]) + in[4];
        loc_fn += in[5];
      }
      s_sum += loc_fp < loc_fn ? loc_fp : loc_fn;
      d_sum += loc_fn > loc_fp ? loc_fn - loc_fp : 0;
      i_sum += loc_fp > loc_fn ? loc_fp - loc_fn : 0;
    }
    rec_sdi[s * 3 + 0] = s_sum;
    rec_sdi[s * 3 + 1] = d_sum;
    rec_sdi[s * 3 + 2] = i_sum;
  }
}

// The five figures from one set of counts; empty denominators give NaN, LE is 180 when nothing was localised.
__device__ __forceinline__ void figures(int64_t nref, int64_t tp, int64_t fps, int64_t fp, int64_t fn, int64_t de_tp,
                                        int64_t de_fn, int64_t sdi, double de, double f[kFigures]) {
  const double f_den = static_cast<double>(tp + fps) + 0.5 * static_cast<double>(fp + fn);
  f[0] = f_den != 0.0 ? static_cast<double>(tp) / f_den : quiet_nan();
  f[1] = nref != 0 ? static_cast<double>(sdi) / static_cast<double>(nref) : quiet_nan();
  f[2] = de_tp != 0 ? de / static_cast<double>(de_tp) : 180.0;
  f[3] = de_tp + de_fn != 0 ? static_cast<double>(de_tp) / static_cast<double>(de_tp + de_fn) : quiet_nan();
  f[4] = (f[1] + (1.0 - f[0]) + f[2] / 180.0 + (1.0 - f[3])) / 4.0;
}

// Lane j <= S: the metrics of every recording but j (j = S: of all).  Classes outermost, so a lane holds one class's
// eleven sums at a time; the kept recordings are added in ascending order.
__global__ __launch_bounds__(kJackThreads) void jackknife_kernel(
    const int64_t* __restrict__ rec_counts, const int64_t* __restrict__ rec_sdi, const double* __restrict__ rec_de, long S,
    double* __restrict__ out, double* __restrict__ out_class) {
  const long j = static_cast<long>(blockIdx.x) * kJackThreads + threadIdx.x;
  if (j > S) return;
  int64_t tot[kSegStats];
#pragma unroll
  for (int i = 0; i < kSegStats; ++i) tot[i] = 0;
  double tot_de = 0.0, macro[kFigures];
#pragma unroll
  for (int i = 0; i < kFigures; ++i) macro[i] = 0.0;
  int n_classes = 0;
  for (int c = 0; c < kC; ++c) {
    int64_t acc[kRecCounts];
#pragma unroll
    for (int i = 0; i < kRecCounts; ++i) acc[i] = 0;
    double de = 0.0;
    for (long s = 0; s < S; ++s) {
      if (s == j) continue;
      const int64_t* in = rec_counts + (s * kC + c) * kRecCounts;
#pragma unroll
      for (int i = 0; i < kRecCounts; ++i) acc[i] += in[i];
      de += rec_de[s * kC + c];
    }
    double f[kFigures];
    figures(acc[0], acc[2], acc[3], acc[4], acc[5], acc[6], acc[7], acc[8] + acc[9] + acc[10], de, f);
    if (acc[0] > 0) {
      n_classes += 1;
#pragma unroll
      for (int i = 0; i < kFigures; ++i) macro[i] += f[i];
    }
    if (j == S) {
#pragma unroll
      for (int i = 0; i < kFigures; ++i) out_class[c * kFigures + i] = f[i];
    }
#pragma unroll
    for (int i = 0; i < kSegStats; ++i) tot[i] += acc[i];
    tot_de += de;
  }
  int64_t sdi = 0;
  for (long s = 0; s < S; ++s) {
    if (s == j) continue;
    sdi += rec_sdi[s * 3 + 0] + rec_sdi[s * 3 + 1] + rec_sdi[s * 3 + 2];
  }
  double micro[kFigures];
  figures(tot[0], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], sdi, tot_de, micro);
  double* o = out + j * 2 * kFigures;
#pragma unroll
  for (int i = 0; i < kFigures; ++i) {
    o[i] = micro[i];
    o[kFigures + i] = n_classes > 0 ? macro[i] / n_classes : quiet_nan();
  }
}

}  // namespace eval
}  // namespace seld

extern "C" {

int seld_doa_assign(const int32_t* det_cell, const float* det_dir, const int32_t* det_count, int K,
                    const int32_t* ref_offsets, const int32_t* ref_dirs, int64_t nq, int I, int J, double thr_deg,
                    double* pair_dist, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  long n_qc = 0;
  unsigned blocks = 0;
  const int rc = check_match_args("seld_doa_assign", det_cell, det_dir, K, nq, I, J, thr_deg >= 0.0,
                                  {det_count, ref_offsets, ref_dirs, pair_dist}, true, &n_qc, &blocks);
  if (rc != kOk || nq == 0) return rc;
  hipLaunchKernelGGL(det_dir ? doa_assign_kernel<true> : doa_assign_kernel<false>, dim3(blocks), dim3(kMatchThreads), 0,
                     static_cast<hipStream_t>(stream_), det_cell, reinterpret_cast<const float2*>(det_dir), det_count, K,
                     ref_offsets, ref_dirs, n_qc, det_dir ? 1 : I, det_dir ? 1 : J, pair_dist);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_segment_score(const double* pair_dist, const int32_t* det_count, int K, const int32_t* ref_offsets,
                       const int64_t* seg_offsets, const int64_t* block_offsets, int64_t S, double thr_deg,
                       int32_t* seg_stats, double* seg_de, int64_t* rec_counts, int64_t* rec_sdi, double* rec_de,
                       void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, "seld_segment_score: K must be in 1..8");
  if (S < 0 || S > 0x7fffffffL || !(thr_deg >= 0.0)) return fail(kErrInvalidArgument, "seld_segment_score: bad extents");
  if (!pair_dist || !det_count || !ref_offsets || !seg_offsets || !block_offsets || !seg_stats || !seg_de || !rec_counts ||
      !rec_sdi || !rec_de)
    return fail(kErrInvalidArgument, "seld_segment_score: null pointer");
  if (S == 0) return kOk;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipLaunchKernelGGL(segment_blocks_kernel, dim3(static_cast<unsigned>(S)), dim3(kSegThreads), 0, stream, pair_dist,
                     det_count, K, ref_offsets, seg_offsets, block_offsets, thr_deg, seg_stats, seg_de);
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(segment_fold_kernel, dim3(static_cast<unsigned>(S)), dim3(kFoldThreads), 0, stream, seg_stats, seg_de,
                     block_offsets, rec_counts, rec_sdi, rec_de);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_jackknife_score(const int64_t* rec_counts, const int64_t* rec_sdi, const double* rec_de, int64_t S, double* out,
                         double* out_class, void* stream_) {
  using namespace seld;
  using namespace seld::eval;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (S < 1 || S > 0x7fffffffL) return fail(kErrInvalidArgument, "seld_jackknife_score: S must be at least 1");
  if (!rec_counts || !rec_sdi || !rec_de || !out || !out_class)
    return fail(kErrInvalidArgument, "seld_jackknife_score: null pointer");
  const long blocks = (static_cast<long>(S) + 1 + kJackThreads - 1) / kJackThreads;
  hipLaunchKernelGGL(jackknife_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kJackThreads), 0,
                     static_cast<hipStream_t>(stream_), rec_counts, rec_sdi, rec_de, static_cast<long>(S), out, out_class);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
