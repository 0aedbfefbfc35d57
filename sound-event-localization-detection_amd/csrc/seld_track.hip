// Track linking of the decoded SELD detections on gfx950: frame-wise peaks -> event tracks with an
// identity over time, gap filling, a minimum duration and onset / offset.
//
// No reference counterpart; the definitions are this project's (section 14.1) and all integer, so the result is exact.
//   track_chain_kernel    one wavefront per chain (segment, class) walks its meta-frames in order.  Lane 8 t + r owns the
//                         pair (slot t, rank r): slot t's state is replicated over its 8 lanes, rank r's detection over
//                         the 8 slots, so a candidate's distance is one LDS lookup per lane and the greedy link is at most
//                         8 rounds of a wave-wide minimum over the keys dist << 6 | t << 3 | r.  Emissions go to a
//                         slot-indexed layout -- entry (frame, slot) of trk_id / trk_cell -- in which every entry is
//                         written exactly once: at its frame when the slot emits or is free, and for the frames a slot
//                         coasts through once its fate is known (the fill when it links again, -1 when it ends).
//   track_compact_kernel  one thread per (frame, class): drops the emissions of tracks shorter than min_len and packs the
//                         rest in ascending id, in place.
// Plain vector stores only, no atomics, a fixed order: the outputs do not depend on how the chains are scheduled.
#include "seld_common.h"
#include "seld_hip.h"

namespace seld {
namespace track {

constexpr int kC = 13;                 // event classes
constexpr int kSlots = 8;              // tracks alive per chain, and emissions per (frame, class)
constexpr int kWave = 64;
constexpr int kMaxGap = 16;
constexpr unsigned kNoKey = 0xffffffffu;
constexpr int kMaxTableBytes = 64 * 1024;

// Minimum over the 64 lanes, every lane active: four DPP steps make each row of 16 lanes uniform (lane ^ 1, lane ^ 2, the
// mirror inside each half row, the mirror of the row), four lane reads and scalar minima join the rows.  No LDS traffic:
// the link loop's latency is this reduction's.
template <int kCtrl>
__device__ __forceinline__ unsigned min_dpp(unsigned v) {
  const unsigned o = static_cast<unsigned>(
      __builtin_amdgcn_update_dpp(static_cast<int>(v), static_cast<int>(v), kCtrl, 0xf, 0xf, false));
  return o < v ? o : v;
}

__device__ __forceinline__ unsigned wave_min(unsigned v) {
  v = min_dpp<0xb1>(v);                                  // quad_perm [1, 0, 3, 2]
  v = min_dpp<0x4e>(v);                                  // quad_perm [2, 3, 0, 1]
  v = min_dpp<0x141>(v);                                 // row_half_mirror
  v = min_dpp<0x140>(v);                                 // row_mirror
  const int x = static_cast<int>(v);
  const unsigned a = static_cast<unsigned>(__builtin_amdgcn_readlane(x, 0));
  const unsigned b = static_cast<unsigned>(__builtin_amdgcn_readlane(x, 16));
  const unsigned c = static_cast<unsigned>(__builtin_amdgcn_readlane(x, 32));
  const unsigned d = static_cast<unsigned>(__builtin_amdgcn_readlane(x, 48));
  const unsigned ab = a < b ? a : b, cd = c < d ? c : d;
  return ab < cd ? ab : cd;
}

// Entries (mm, slot t) for mm in [a, b), b - a <= kMaxGap + 1, shared among the 8 lanes of slot t.
__device__ __forceinline__ void write_span(int32_t* __restrict__ ids, int32_t* __restrict__ cells, long base_q, int c,
                                           int t, int r, int a, int b, int id, int cell) {
#pragma unroll
  for (int k = 0; k < (kMaxGap + 1 + kSlots - 1) / kSlots; ++k) {
    const int mm = a + r + kSlots * k;
    if (mm < b) {
      const long e = ((base_q + mm) * kC + c) * kSlots + t;
      ids[e] = id;
      cells[e] = cell;
    }
  }
}

__global__ __launch_bounds__(kWave) void track_chain_kernel(
    const int32_t* __restrict__ det_cell, const int32_t* __restrict__ det_count, int K,
    const int64_t* __restrict__ seg_offsets, const int32_t* __restrict__ table, int I, int J, int gate, int max_gap,
    int min_len, const int64_t* __restrict__ chain_offsets, int32_t* __restrict__ trk_cell, int32_t* __restrict__ trk_id,
    int32_t* __restrict__ tracks, int32_t* __restrict__ chain_tracks) {
  extern __shared__ int32_t dist[];                      // [I][I][J]
  const int lane = threadIdx.x;
  const int t = lane >> 3, r = lane & 7;
  const int x = blockIdx.x;                              // chain = segment * 13 + class
  const int s = x / kC, c = x - s * kC;
  const long q_lo = seg_offsets[s];
  const int M = static_cast<int>(seg_offsets[s + 1] - q_lo);
  const long row0 = chain_offsets[x];
  const int row_cap = static_cast<int>(chain_offsets[x + 1] - row0);   // upper bound on this chain's tracks
  const int n_cells = I * J;
  for (int e = lane; e < I * n_cells; e += kWave) dist[e] = table[e];
  __syncthreads();

  // slot t, replicated over its 8 lanes (id < 0: free)
  int id = -1, cell = 0, ci = 0, cj = 0, first = 0, last = 0, seen = 0;
  int next_id = 0;

  auto close_track = [&]() {                             // the slot's track ends: its record, by the slot's first lane
    if (r == 0 && id < row_cap) {
      int4 rec;
      rec.x = first;
      rec.y = last;
      rec.z = seen;
      rec.w = (last - first + 1 >= min_len) ? 1 : 0;
      reinterpret_cast<int4*>(tracks)[row0 + id] = rec;
    }
  };

  // the detections of frame m for rank r (replicated over t), read one frame ahead
  int nx_cell = -1, nx_count = 0;
  if (M > 0) {
    nx_count = det_count[q_lo * kC + c];
    nx_cell = r < K ? det_cell[(q_lo * kC + c) * K + r] : -1;
  }
  for (int m = 0; m < M; ++m) {
    const int d_cell = nx_cell;
    int cnt = nx_count;
    if (m + 1 < M) {
      nx_count = det_count[(q_lo + m + 1) * kC + c];
      nx_cell = r < K ? det_cell[((q_lo + m + 1) * kC + c) * K + r] : -1;
    }
    cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
    // n = detections up to the first cell outside the grid
    const bool bad = r >= cnt || d_cell < 0 || d_cell >= n_cells;
    const unsigned bad8 = static_cast<unsigned>(__ballot(bad)) & 0xffu;          // lanes 0..7: slot 0's copy of the ranks
    const int n = __ffs(static_cast<int>(bad8 | 0x100u)) - 1;
    const int di = d_cell / J, dj = d_cell - di * J;

    // 1. expire
    if (id >= 0 && m - last > max_gap + 1) {
      write_span(trk_id, trk_cell, q_lo, c, t, r, last + 1, m, -1, -1);
      close_track();
      id = -1;
    }
    // 2. candidates
    unsigned key = kNoKey;
    if (id >= 0 && r < n) {
      int dd = dj - cj;
      dd = dd < 0 ? dd + J : dd;
      const int d = dist[(ci * I + di) * J + dd];
      if (d <= gate) key = (static_cast<unsigned>(d) << 6) | static_cast<unsigned>(lane);
    }
    // 3. greedy link
    unsigned linked_slots = 0, linked_ranks = 0;
    for (int round = 0; round < kSlots; ++round) {
      const unsigned best = wave_min(key);
      if (best == kNoKey) break;
      const int bt = (best >> 3) & 7, br = best & 7;
      const int new_cell = __builtin_amdgcn_readlane(d_cell, br);                 // lane br = (slot 0, rank br)
      linked_slots |= 1u << bt;
      linked_ranks |= 1u << br;
      if (t == bt) {
        write_span(trk_id, trk_cell, q_lo, c, t, r, last + 1, m, id, cell);    // the fill, with the cell before the update
        cell = new_cell;
        ci = cell / J;
        cj = cell - ci * J;
        last = m;
        ++seen;
        write_span(trk_id, trk_cell, q_lo, c, t, r, m, m + 1, id, cell);
      }
      if (t == bt || r == br) key = kNoKey;
    }
    // 4. births, in rank order
    for (int br = 0; br < n; ++br) {
      if ((linked_ranks >> br) & 1u) continue;
      const int new_cell = __builtin_amdgcn_readlane(d_cell, br);
      const unsigned long long free_lanes = __ballot(id < 0);
      int bt;
      if (free_lanes) {
        bt = (__ffsll(static_cast<long long>(free_lanes)) - 1) >> 3;
      } else {                                           // all 8 occupied: the unlinked slot last seen longest ago
        const bool cand = r == 0 && !((linked_slots >> t) & 1u);
        const unsigned k2 = wave_min(cand ? (static_cast<unsigned>(last) << 3) | static_cast<unsigned>(t) : kNoKey);
        bt = k2 & 7;
      }
      if (t == bt) {
        if (id >= 0) {                                   // that track ends here
          write_span(trk_id, trk_cell, q_lo, c, t, r, last + 1, m, -1, -1);
          close_track();
        }
        id = next_id;
        cell = new_cell;
        ci = cell / J;
        cj = cell - ci * J;
        first = last = m;
        seen = 1;
        write_span(trk_id, trk_cell, q_lo, c, t, r, m, m + 1, id, cell);
      }
      ++next_id;
    }
    // a slot free at the end of the frame emits nothing there
    if (id < 0) write_span(trk_id, trk_cell, q_lo, c, t, r, m, m + 1, -1, -1);
  }
  if (id >= 0) {                                         // the chain ends: so does every track still alive
    write_span(trk_id, trk_cell, q_lo, c, t, r, last + 1, M, -1, -1);
    close_track();
  }
  if (lane == 0) chain_tracks[x] = next_id;
}

// One thread per (frame m, class c) of chain blockIdx.x, frames strided over the block.
__global__ __launch_bounds__(kWave) void track_compact_kernel(
    const int64_t* __restrict__ seg_offsets, const int64_t* __restrict__ chain_offsets,
    const int32_t* __restrict__ tracks, int32_t* __restrict__ trk_cell, int32_t* __restrict__ trk_id,
    int32_t* __restrict__ trk_count) {
  const int x = blockIdx.x;
  const int s = x / kC, c = x - s * kC;
  const long q_lo = seg_offsets[s];
  const int M = static_cast<int>(seg_offsets[s + 1] - q_lo);
  const long row0 = chain_offsets[x];
  const int row_cap = static_cast<int>(chain_offsets[x + 1] - row0);
  for (int m = threadIdx.x; m < M; m += kWave) {
    const long qc = (q_lo + m) * kC + c;
    int4* ids4 = reinterpret_cast<int4*>(trk_id + qc * kSlots);
    int4* cells4 = reinterpret_cast<int4*>(trk_cell + qc * kSlots);
    const int4 ia = ids4[0], ib = ids4[1], ca = cells4[0], cb = cells4[1];
    int ids[kSlots] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
    const int cells[kSlots] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
    for (int t = 0; t < kSlots; ++t) {
      const bool live = ids[t] >= 0 && ids[t] < row_cap;
      const int kept = live ? tracks[(row0 + ids[t]) * 4 + 3] : 0;
      ids[t] = kept ? ids[t] : -1;
    }
    int pos[kSlots];
    int count = 0;
#pragma unroll
    for (int t = 0; t < kSlots; ++t) {
      int p = 0;
#pragma unroll
      for (int u = 0; u < kSlots; ++u) p += (ids[u] >= 0 && ids[u] < ids[t]) ? 1 : 0;     // ids are distinct
      pos[t] = ids[t] >= 0 ? p : -1;
      count += ids[t] >= 0 ? 1 : 0;
    }
    int out_id[kSlots], out_cell[kSlots];
#pragma unroll
    for (int p = 0; p < kSlots; ++p) {
      int oi = -1, oc = -1;
#pragma unroll
      for (int t = 0; t < kSlots; ++t) {
        oi = pos[t] == p ? ids[t] : oi;
        oc = pos[t] == p ? cells[t] : oc;
      }
      out_id[p] = oi;
      out_cell[p] = oc;
    }
    ids4[0] = make_int4(out_id[0], out_id[1], out_id[2], out_id[3]);
    ids4[1] = make_int4(out_id[4], out_id[5], out_id[6], out_id[7]);
    cells4[0] = make_int4(out_cell[0], out_cell[1], out_cell[2], out_cell[3]);
    cells4[1] = make_int4(out_cell[4], out_cell[5], out_cell[6], out_cell[7]);
    trk_count[qc] = count;
  }
}

}  // namespace track
}  // namespace seld

extern "C" {

int seld_track_link(const int32_t* det_cell, const int32_t* det_count, int K, const int64_t* seg_offsets, int64_t S,
                    const int32_t* dist_table, int I, int J, int gate_mdeg, int max_gap, int min_len,
                    const int64_t* chain_offsets, int32_t* trk_cell, int32_t* trk_id, int32_t* trk_count, int32_t* tracks,
                    int32_t* chain_tracks, void* stream_) {
  using namespace seld;
  using namespace seld::track;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (K < 1 || K > kSlots) return fail(kErrInvalidArgument, "seld_track_link: K must be in 1..8");
  if (max_gap < 0 || max_gap > kMaxGap) return fail(kErrInvalidArgument, "seld_track_link: max_gap must be in 0..16");
  if (min_len < 1) return fail(kErrInvalidArgument, "seld_track_link: min_len must be >= 1");
  if (gate_mdeg < 0) return fail(kErrInvalidArgument, "seld_track_link: gate_mdeg must be >= 0");
  if (S < 0 || I < 1 || J < 1) return fail(kErrInvalidArgument, "seld_track_link: bad extents");
  if (!det_cell || !det_count || !seg_offsets || !dist_table || !chain_offsets || !trk_cell || !trk_id || !trk_count ||
      !tracks || !chain_tracks)
    return fail(kErrInvalidArgument, "seld_track_link: null pointer");
  const long table_bytes = static_cast<long>(I) * I * J * static_cast<long>(sizeof(int32_t));
  if (table_bytes > kMaxTableBytes)
    return fail(kErrUnsupported, "seld_track_link: the distance table must fit in 64 KB of LDS (I * I * J <= 16384)");
  if (((reinterpret_cast<uintptr_t>(trk_cell) | reinterpret_cast<uintptr_t>(trk_id) | reinterpret_cast<uintptr_t>(tracks)) &
       15u) != 0)
    return fail(kErrUnsupported, "seld_track_link: trk_cell, trk_id and tracks must be 16-byte aligned");
  if (S == 0) return kOk;
  if (S * kC > 0x7fffffffLL) return fail(kErrUnsupported, "seld_track_link: too many chains for one launch");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned chains = static_cast<unsigned>(S * kC);
  hipLaunchKernelGGL(track_chain_kernel, dim3(chains), dim3(kWave), static_cast<size_t>(table_bytes), stream, det_cell,
                     det_count, K, seg_offsets, dist_table, I, J, gate_mdeg, max_gap, min_len, chain_offsets, trk_cell,
                     trk_id, tracks, chain_tracks);
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(track_compact_kernel, dim3(chains), dim3(kWave), 0, stream, seg_offsets, chain_offsets, tracks,
                     trk_cell, trk_id, trk_count);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
