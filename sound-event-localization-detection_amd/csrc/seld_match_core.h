// The location-aware matching behind seld_doa_match (seld_eval.hip), seld_doa_match_dirs (seld_refine.hip),
// seld_doa_match_prefix (seld_sweep.hip) and seld_doa_assign (seld_segment.hip), DESIGN.md sections 10.2, 15, 17, 18 and 20.
// Shared by all four, so they cannot drift apart in a distance, a comparison or a check:
//   det_direction<kDirs>         detection p's direction in float64: its float (az, el) or the centre of its cell
//   fill_distances<kDirs>        the reference x detection distances into LDS; returns the within-threshold mask `adj`
//   refused                      the (nr, np) an entry must have for the bodies to stay inside their tables
//   min_cost_assignment<kChoice> the dp over column masks; with kChoice also the choice table and the best mask
//   check_match_args             the host prologue of the four entry points
// match_entry<kDirs> is the whole body of the first two kernels, match_prefix_entry<kDirs> of the third (its two walks read
// the dp's layers, so they keep their own loops), assign_entry<kDirs> of the fourth.
#pragma once

#include <initializer_list>

#include "seld_common.h"
#include "seld_eval_core.h"

namespace seld {
namespace eval {

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

using Lanes = double[kMatchThreads];                   // one LDS row: a value per lane of the workgroup

// An entry the host refuses (more than 8 references, a count outside 0..K): the bodies write their "refused" outputs
// and never read out of range.
__device__ __forceinline__ bool refused(int nr, int np, int K) { return nr < 0 || nr > kMaxSide || np < 0 || np > K; }

// Detection `at` (= qc * K + p): with kDirs its direction det_dir[at] = (az, el) degrees, widened to float64 (det_cell, I,
// J unused); else the centre of cell det_cell[at] of the I x J grid (det_dir unused).
template <bool kDirs>
__device__ __forceinline__ void det_direction(const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir,
                                              long at, int I, int J, double& az, double& el) {
  if constexpr (kDirs) {
    const float2 dir = det_dir[at];
    az = static_cast<double>(dir.x);
    el = static_cast<double>(dir.y);
  } else {
    const double cell_az = 360.0 / J, cell_el = 180.0 / I;
    const int cell = det_cell[at];
    const int ci = cell / J, cj = cell - ci * J;
    az = -180.0 + (cj + 0.5) * cell_az;
    el = -90.0 + (ci + 0.5) * cell_el;
  }
}

// dist[row * 8 + col][lane] = distance of reference r (r0 + r of ref_dirs) to detection p of entry qc, for r < nr, p < np;
// (row, col) = (r, p) with refs_are_rows, else (p, r).  Returns adj: bit 8 r + p set when that distance is <= thr_deg.
template <bool kDirs>
__device__ __forceinline__ uint64_t fill_distances(const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir,
                                                   long qc, int K, const int32_t* __restrict__ ref_dirs, int r0, int nr,
                                                   int np, int I, int J, double thr_deg, bool refs_are_rows, Lanes* dist,
                                                   int lane) {
  uint64_t adj = 0;
  for (int r = 0; r < nr; ++r) {
    const double raz = ref_dirs[2 * (r0 + r)], rel = ref_dirs[2 * (r0 + r) + 1];
    for (int p = 0; p < np; ++p) {
      double az, el;
      det_direction<kDirs>(det_cell, det_dir, qc * K + p, I, J, az, el);
      const double d = angle_deg(raz, rel, az, el);
      if (d <= thr_deg) adj |= 1ull << (8 * r + p);
      dist[refs_are_rows ? r * kMaxSide + p : p * kMaxSide + r][lane] = d;
    }
  }
  return adj;
}

// The minimum total distance of an injection of rows 0..k-1 into `cols` columns (k <= cols): dp over the sets of used
// columns in ascending mask order, row = popcount - 1, a mask's candidates its set bits in ascending order; 0 when k is 0.
// kChoice: choice[mask][lane] is the column that set dp[mask] and *best_mask the first mask of k columns with the minimum
// (the k lowest columns when no candidate compares: NaN directions), for a backtrack.
template <bool kChoice>
__device__ __forceinline__ double min_cost_assignment(const Lanes* dist, Lanes* dp, int lane, int k, int cols,
                                                      uint8_t (*choice)[kMatchThreads] = nullptr,
                                                      uint32_t* best_mask = nullptr) {
  if (k == 0) return 0.0;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double best = inf;
  if constexpr (kChoice) *best_mask = (1u << k) - 1u;
  dp[0][lane] = 0.0;
  for (uint32_t mask = 1; mask < (1u << cols); ++mask) {
    const int pc = __popc(mask);
    if (pc > k) continue;
    const int r = pc - 1;
    double v = inf;
    [[maybe_unused]] int pick = __ffs(mask) - 1;                  // (always a set bit, so a backtrack stays inside the mask)
    for (int b = 0; b < cols; ++b) {
      if (!((mask >> b) & 1u)) continue;
      const double cand = dp[mask ^ (1u << b)][lane] + dist[r * kMaxSide + b][lane];
      if (cand < v) {
        v = cand;
        if constexpr (kChoice) pick = b;
      }
    }
    dp[mask][lane] = v;
    if constexpr (kChoice) choice[mask][lane] = static_cast<uint8_t>(pick);
    if (pc == k && v < best) {
      best = v;
      if constexpr (kChoice) *best_mask = mask;
    }
  }
  return best;
}

// One lane's (q, c) entry of a workgroup of kMatchThreads lanes.  The kernel's only LDS is declared here.
template <bool kDirs>
__device__ __forceinline__ void match_entry(const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir,
                                            const int32_t* __restrict__ det_count, int K,
                                            const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs,
                                            long n_qc, int I, int J, double thr_deg, int32_t* __restrict__ stats,
                                            double* __restrict__ cost) {
  __shared__ double dist[kMaxSide * kMaxSide][kMatchThreads];    // [row][col], lane-minor: no bank conflicts
  __shared__ double dp[1 << kMaxSide][kMatchThreads];            // minimum cost per set of used columns
  const int lane = threadIdx.x;
  const long qc = static_cast<long>(blockIdx.x) * kMatchThreads + lane;
  if (qc >= n_qc) return;                                         // (no barriers below)
  const int r0 = ref_offsets[qc];
  const int nr = ref_offsets[qc + 1] - r0;
  const int np = det_count[qc];
  int32_t* st = stats + qc * 4;
  if (refused(nr, np, K)) {
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
  const uint64_t adj = fill_distances<kDirs>(det_cell, det_dir, qc, K, ref_dirs, r0, nr, np, I, J, thr_deg, refs_are_rows,
                                             dist, lane);
  // tp = maximum matching within the threshold = min over reference sets S of (nr - |S| + |N(S)|) (Hall / Koenig)
  int tp = nr < np ? nr : np;
  for (uint32_t s = 1; s < (1u << nr); ++s) {
    uint32_t nb = 0;
    for (int r = 0; r < nr; ++r)
      if ((s >> r) & 1u) nb |= static_cast<uint32_t>(adj >> (8 * r)) & 0xffu;
    const int v = nr - __popc(s) + __popc(nb);
    tp = v < tp ? v : tp;
  }
  const double best = min_cost_assignment<false>(dist, dp, lane, rows, cols);
  st[0] = nr;
  st[1] = np;
  st[2] = rows;
  st[3] = tp;
  cost[qc] = best;
}

// seld_doa_assign's body: the assignment ITSELF.  pair_dist [n_qc][8]: slot r is the distance of reference r to the
// detection match_entry's minimum-cost assignment gives it, NaN when unassigned, absent or the entry refused.  No threshold:
// fill_distances' mask is dropped, and with it the comparison.
template <bool kDirs>
__device__ __forceinline__ void assign_entry(const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir,
                                             const int32_t* __restrict__ det_count, int K,
                                             const int32_t* __restrict__ ref_offsets, const int32_t* __restrict__ ref_dirs,
                                             long n_qc, int I, int J, double* __restrict__ pair_dist) {
  __shared__ double dist[kMaxSide * kMaxSide][kMatchThreads];    // [row][col], lane-minor: no bank conflicts
  __shared__ double dp[1 << kMaxSide][kMatchThreads];            // minimum cost per set of used columns
  __shared__ uint8_t choice[1 << kMaxSide][kMatchThreads];       // the column that set dp[mask]
  const int lane = threadIdx.x;
  const long qc = static_cast<long>(blockIdx.x) * kMatchThreads + lane;
  if (qc >= n_qc) return;                                         // (no barriers below)
  double* out = pair_dist + qc * kMaxSide;
#pragma unroll
  for (int r = 0; r < kMaxSide; ++r) out[r] = __longlong_as_double(0x7ff8000000000000LL);
  const int r0 = ref_offsets[qc];
  const int nr = ref_offsets[qc + 1] - r0;
  const int np = det_count[qc];
  if (refused(nr, np, K)) return;                                 // all NaN
  const bool refs_are_rows = nr <= np;
  const int rows = refs_are_rows ? nr : np, cols = refs_are_rows ? np : nr;
  fill_distances<kDirs>(det_cell, det_dir, qc, K, ref_dirs, r0, nr, np, I, J, 0.0, refs_are_rows, dist, lane);
  if (rows == 0) return;
  uint32_t mask = 0;
  min_cost_assignment<true>(dist, dp, lane, rows, cols, choice, &mask);
  for (int row = rows - 1; row >= 0; --row) {
    const int b = choice[mask][lane];
    out[refs_are_rows ? row : b] = dist[row * kMaxSide + b][lane];
    mask ^= 1u << b;
  }
}

// ---- every prefix of an entry at once (seld_doa_match_prefix, seld_sweep.hip) ---------------------
// ptp / pcost [n_qc][K + 1]: entry p <= min(np, K) holds the tp and cost match_entry writes when det_count[qc] is replaced
// by p; entries past the count repeat the one at the count.  The additions are match_entry's, in its order:
//   p <  nr  the detections are match_entry's rows.  ONE dp over the sets of used references; dp[mask] sums rows
//            0..popcount - 1, so the cost of prefix p is the minimum of the popcount-p layer (match_entry with count p runs
//            the same recurrence and only skips the layers above p).
//   p >= nr  the references are the rows.  ONE dp over the sets of used detections; match_entry with count p visits the
//            masks below 2^p in ascending order, so the cost of prefix p is the running minimum of the popcount-nr layer
//            when the walk reaches mask 2^p - 1.  (The candidates of a mask are its set bits in ascending order whatever
//            the column count.)
// tp of prefix p: the Hall / Koenig minimum with every neighbourhood masked to the first p detections.
constexpr int kPrefixes = kMaxSide + 1;

template <bool kDirs>
__device__ __forceinline__ void match_prefix_entry(const int32_t* __restrict__ det_cell, const float2* __restrict__ det_dir,
                                                   const int32_t* __restrict__ det_count, int K,
                                                   const int32_t* __restrict__ ref_offsets,
                                                   const int32_t* __restrict__ ref_dirs, long n_qc, int I, int J,
                                                   double thr_deg, int32_t* __restrict__ ptp, double* __restrict__ pcost) {
  __shared__ double dist[kMaxSide * kMaxSide][kMatchThreads];    // [reference r][detection p], lane-minor
  __shared__ double dp[1 << kMaxSide][kMatchThreads];            // minimum cost per set of used columns (both walks)
  __shared__ double layer[kPrefixes][kMatchThreads];             // cost per prefix
  const int lane = threadIdx.x;
  const long qc = static_cast<long>(blockIdx.x) * kMatchThreads + lane;
  if (qc >= n_qc) return;                                         // (no barriers below)
  const int r0 = ref_offsets[qc];
  const int nr = ref_offsets[qc + 1] - r0;
  const int np = det_count[qc];
  int32_t* tp_out = ptp + qc * (K + 1);
  double* cost_out = pcost + qc * (K + 1);
  if (refused(nr, np, K)) {
    for (int p = 0; p <= K; ++p) {
      tp_out[p] = -1;
      cost_out[p] = __longlong_as_double(0x7ff8000000000000LL);
    }
    return;
  }
  const uint64_t adj = fill_distances<kDirs>(det_cell, det_dir, qc, K, ref_dirs, r0, nr, np, I, J, thr_deg, true, dist, lane);
  // tp[p] = min over reference sets S of (nr - |S| + |N(S) among the first p detections|); p > np repeats np
  int tp[kPrefixes];
#pragma unroll
  for (int p = 0; p < kPrefixes; ++p) {
    const int pp = p < np ? p : np;
    tp[p] = nr < pp ? nr : pp;
  }
  for (uint32_t s = 1; s < (1u << nr); ++s) {
    uint32_t nb = 0;
    for (int r = 0; r < nr; ++r)
      if ((s >> r) & 1u) nb |= static_cast<uint32_t>(adj >> (8 * r)) & 0xffu;
    const int base = nr - __popc(s);
#pragma unroll
    for (int p = 0; p < kPrefixes; ++p) {
      const int v = base + __popc(nb & ((1u << p) - 1u));
      tp[p] = v < tp[p] ? v : tp[p];
    }
  }
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  for (int p = 0; p < kPrefixes; ++p) layer[p][lane] = (nr == 0 || p == 0) ? 0.0 : inf;
  // prefixes 1 .. min(np, nr - 1): rows = detections, columns = references
  const int ka = np < nr - 1 ? np : nr - 1;
  if (ka >= 1) {
    dp[0][lane] = 0.0;
    for (uint32_t mask = 1; mask < (1u << nr); ++mask) {
      const int pc = __popc(mask);
      if (pc > ka) continue;
      const int row = pc - 1;
      double v = inf;
      for (int b = 0; b < nr; ++b) {
        if (!((mask >> b) & 1u)) continue;
        const double cand = dp[mask ^ (1u << b)][lane] + dist[b * kMaxSide + row][lane];
        v = cand < v ? cand : v;
      }
      dp[mask][lane] = v;
      const double cur = layer[pc][lane];
      layer[pc][lane] = v < cur ? v : cur;
    }
  }
  // prefixes nr .. np: rows = references, columns = detections
  if (nr >= 1 && np >= nr) {
    dp[0][lane] = 0.0;
    double best = inf;
    for (uint32_t mask = 1; mask < (1u << np); ++mask) {
      const int pc = __popc(mask);
      if (pc <= nr) {
        const int row = pc - 1;
        double v = inf;
        for (int b = 0; b < np; ++b) {
          if (!((mask >> b) & 1u)) continue;
          const double cand = dp[mask ^ (1u << b)][lane] + dist[row * kMaxSide + b][lane];
          v = cand < v ? cand : v;
        }
        dp[mask][lane] = v;
        if (pc == nr) best = v < best ? v : best;
      }
      if ((mask & (mask + 1u)) == 0 && pc >= nr) layer[pc][lane] = best;     // mask = 2^pc - 1: prefix pc is complete
    }
  }
#pragma unroll
  for (int p = 0; p < kPrefixes; ++p) {
    if (p <= K) {
      tp_out[p] = tp[p];
      cost_out[p] = layer[p < np ? p : np][lane];
    }
  }
}

// ---- the host prologue of the four entry points ------------------------------------------------------------------------
// The detections are named by det_dir when it is given, else by det_cell on the I x J grid.  In this order: the library's
// state, K, the extents (nq; I and J for cells; `extra_ok`, an entry point's own condition), the empty call, the pointers
// (the detections and `others`), det_dir's alignment, the launch limit.  `nulls_first`: the pointers are looked at before
// the empty call (seld_doa_assign).  Returns kOk with *n_qc and *blocks set; a caller launches nothing when the code is
// not kOk or nq is 0.
inline int check_match_args(const char* who, const int32_t* det_cell, const float* det_dir, int K, int64_t nq, int I, int J,
                            bool extra_ok, std::initializer_list<const void*> others, bool nulls_first, long* n_qc,
                            unsigned* blocks) {
  const std::string name(who);
  if (!current_state()) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, name + ": K must be in 1..8");
  if (nq < 0 || (!det_dir && (I < 1 || J < 1)) || !extra_ok) return fail(kErrInvalidArgument, name + ": bad extents");
  if (nq == 0 && !nulls_first) return kOk;
  if (!det_cell && !det_dir) return fail(kErrInvalidArgument, name + ": null pointer");
  for (const void* ptr : others)
    if (!ptr) return fail(kErrInvalidArgument, name + ": null pointer");
  if (nq == 0) return kOk;
  if (det_dir && (reinterpret_cast<uintptr_t>(det_dir) & 7u) != 0)
    return fail(kErrUnsupported, name + ": det_dir must be 8-byte aligned");
  *n_qc = static_cast<long>(nq) * kC;
  const long n_blocks = (*n_qc + kMatchThreads - 1) / kMatchThreads;
  if (n_blocks > 0x7fffffffL) return fail(kErrUnsupported, name + ": too many meta-frames for one launch");
  *blocks = static_cast<unsigned>(n_blocks);
  return kOk;
}

}  // namespace eval
}  // namespace seld
