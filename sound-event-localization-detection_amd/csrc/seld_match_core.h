// The location-aware matching shared by seld_doa_match (seld_eval.hip: detections are grid cells) and seld_doa_match_dirs
// (seld_refine.hip: detections are float directions), DESIGN.md sections 10.2 and 15.  match_entry<kDirs> is the whole
// kernel body; the two entry points differ only in the `if constexpr (kDirs)` that names detection p's direction in
// float64, so they cannot drift apart in the distance, the matching or the assignment.  match_prefix_entry<kDirs> below is
// the body of seld_doa_match_prefix (seld_sweep.hip): the same distances and additions for every prefix of an entry at once.
#pragma once

#include "seld_common.h"

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

// One lane's (q, c) entry of a workgroup of kMatchThreads lanes.  Detection p of entry qc: with kDirs its direction
// det_dir[qc * K + p] = (az, el) degrees, widened to float64 (det_cell, I, J unused); else the centre of cell
// det_cell[qc * K + p] of the I x J grid (det_dir unused).  The kernel's only LDS is declared here.
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
  [[maybe_unused]] const double cell_az = 360.0 / J, cell_el = 180.0 / I;
  for (int r = 0; r < nr; ++r) {
    const double raz = ref_dirs[2 * (r0 + r)], rel = ref_dirs[2 * (r0 + r) + 1];
    for (int p = 0; p < np; ++p) {
      double d;
      if constexpr (kDirs) {
        const float2 dir = det_dir[qc * K + p];
        d = angle_deg(raz, rel, static_cast<double>(dir.x), static_cast<double>(dir.y));
      } else {
        const int cell = det_cell[qc * K + p];
        const int ci = cell / J, cj = cell - ci * J;
        d = angle_deg(raz, rel, -180.0 + (cj + 0.5) * cell_az, -90.0 + (ci + 0.5) * cell_el);
      }
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
  if (nr < 0 || nr > kMaxSide || np < 0 || np > K) {             // refused, as match_entry refuses it
    for (int p = 0; p <= K; ++p) {
      tp_out[p] = -1;
      cost_out[p] = __longlong_as_double(0x7ff8000000000000LL);
    }
    return;
  }
  uint64_t adj = 0;                                               // bit 8 r + p: reference r within thr of detection p
  [[maybe_unused]] const double cell_az = 360.0 / J, cell_el = 180.0 / I;
  for (int r = 0; r < nr; ++r) {
    const double raz = ref_dirs[2 * (r0 + r)], rel = ref_dirs[2 * (r0 + r) + 1];
    for (int p = 0; p < np; ++p) {
      double d;
      if constexpr (kDirs) {
        const float2 dir = det_dir[qc * K + p];
        d = angle_deg(raz, rel, static_cast<double>(dir.x), static_cast<double>(dir.y));
      } else {
        const int cell = det_cell[qc * K + p];
        const int ci = cell / J, cj = cell - ci * J;
        d = angle_deg(raz, rel, -180.0 + (cj + 0.5) * cell_az, -90.0 + (ci + 0.5) * cell_el);
      }
      if (d <= thr_deg) adj |= 1ull << (8 * r + p);
      dist[r * kMaxSide + p][lane] = d;
    }
  }
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

}  // namespace eval
}  // namespace seld
