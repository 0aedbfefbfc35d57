// The grid-map decode shared by seld_grid_decode (seld_eval.hip), seld_grid_decode_tta (seld_tta.hip) and
// seld_grid_decode_refine (seld_refine.hip): one meta-frame per workgroup of 512 threads, DESIGN.md sections 10, 13, 15
// and 20.  Shared by all three, so they cannot drift apart in summation order, arithmetic or a check:
//   decode_meta_frame<kBf16, kTta, kRefine>  the whole kernel body; with kTta = false every `if constexpr (kTta)` drops out
//                                            and what is left is the plain decode, and with kRefine = false so does the
//                                            sub-cell DOA epilogue
//   check_decode_args, pack_patterns         the host prologue of the three entry points
//   launch_meta_frames                       their launch: one workgroup per meta-frame
#pragma once

#include "seld_common.h"

namespace seld {
namespace eval {

constexpr int kI = 18, kJ = 36, kCells = kI * kJ;      // 10-degree grid, cell = i * J + j (utils.py:77-90)
constexpr int kM = 14, kC = 13;                        // 13 event classes + background
constexpr int kWin = 250, kHop = 50;                   // windows of the timeline (dataset.py:267-317)
constexpr int kRowElems = kCells * kM;                 // 9 072 logits per (window, frame)
constexpr int kThreads = 512;                         // 8 waves: two per SIMD hide each other's latency
constexpr int kCellsPerThread = (kCells + kThreads - 1) / kThreads;   // 2
constexpr int kMaxK = 8;
constexpr int kProbFloats = kCells * kC;               // 8 424: P_q of one meta-frame
constexpr int kMaxPatterns = 16;                       // the sign-and-swap transforms of the FOA channels (section 11.1)

template <bool kBf16> struct Row {
  static constexpr int kBytes = kRowElems * (kBf16 ? 2 : 4);
  static constexpr int kChunks = kBytes / 16;                              // 1 134 (bf16) / 2 268 (fp32)
  static constexpr int kPerThread = (kChunks + kThreads - 1) / kThreads;  // 3 / 5
  // LDS: one staged row, reused for P_q once the rows are consumed
  static constexpr int kLdsChunks = kChunks > kProbFloats / 4 ? kChunks : kProbFloats / 4;
};
static_assert(kRowElems * 2 % 16 == 0, "bf16 rows must be whole 16-byte chunks");
static_assert(kProbFloats % 4 == 0, "P_q must be whole 16-byte chunks");
static_assert(kJ % 4 == 0, "a quarter turn must be a whole number of cells");

// Windows covering frame f: HOP*w <= f < HOP*w + WIN, 0 <= w < W.
__device__ __forceinline__ long first_window(long f) { return f < kWin ? 0 : (f - kWin) / kHop + 1; }
__device__ __forceinline__ long last_window(long f, long W) { const long w = f / kHop; return w < W - 1 ? w : W - 1; }

// 14 logits of one cell from the staged row -> the 13 event-class probabilities (softmax in fp32)
template <bool kBf16> __device__ __forceinline__ void cell_softmax(const uint4* stage, int cell, float p[kC]) {
  float x[kM];
  if constexpr (kBf16) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(stage) + cell * (kM / 2);   // 28 B per cell, 4-byte aligned
#pragma unroll
    for (int e = 0; e < kM / 2; ++e) {
      const uint32_t v = w[e];
      x[2 * e] = __uint_as_float(v << 16);
      x[2 * e + 1] = __uint_as_float(v & 0xffff0000u);
    }
  } else {
    const float2* w = reinterpret_cast<const float2*>(stage) + cell * (kM / 2);       // 56 B per cell, 8-byte aligned
#pragma unroll
    for (int e = 0; e < kM / 2; ++e) {
      const float2 v = w[e];
      x[2 * e] = v.x;
      x[2 * e + 1] = v.y;
    }
  }
  float m = x[0];
#pragma unroll
  for (int k = 1; k < kM; ++k) m = fmaxf(m, x[k]);
  // hardware exp2 and one reciprocal per cell: a few ulp of fp32, far inside the 2e-5 the decode is held to, and the
  // row's arithmetic no longer outlasts its loads
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kM; ++k) {
    x[k] = __expf(x[k] - m);
    s += x[k];
  }
  const float inv = 1.0f / s;
#pragma unroll
  for (int k = 0; k < kC; ++k) p[k] = x[k] * inv;
}

// (score, cell) order of the detections: score descending, then cell ascending; cell == kCells marks "none"
__device__ __forceinline__ bool before(float sa, int ca, float sb, int cb) {
  if (cb == kCells) return ca != kCells;
  if (ca == kCells) return false;
  return sa > sb || (sa == sb && ca < cb);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // (HIP's uint4 wrapper keeps arrays of it in scratch)

// this thread's 16-byte chunks of row (window wi, frame fr) into registers
template <bool kBf16>
__device__ __forceinline__ void load_row(const uint4* __restrict__ logits, long w0, long fr, long wi, int tid,
                                         u32x4 (&next)[Row<kBf16>::kPerThread]) {
  using R = Row<kBf16>;
  const u32x4* src = reinterpret_cast<const u32x4*>(logits) + ((wi - w0) * kWin + (fr - kHop * wi)) * static_cast<long>(R::kChunks);
#pragma unroll
  for (int e = 0; e < R::kPerThread; ++e) {
    const int ch = tid + e * kThreads;
    if (ch < R::kChunks) next[e] = src[ch];
  }
}

// Where the event of original cell (i, j) shows in the maps of a window gathered with spatial pattern p (seld_augment
// cell_dest): mirror p >> 3, then (p >> 1) & 3 quarter turns, then elevation flip p & 1.  p is wave-uniform.
__device__ __forceinline__ int cell_dest(int i, int j, int p) {
  const int i2 = (p & 1) ? kI - 1 - i : i;
  int j2 = ((p & 8) ? kJ - 1 - j : j) + ((p >> 1) & 3) * (kJ / 4);
  j2 = j2 >= kJ ? j2 - kJ : j2;
  return i2 * kJ + j2;
}

// Sub-cell DOA of the detection of class c at peak cell x (section 15.1): v = sum over x and its up-to-8 neighbours y
// (the peak test's rule) of P_q[y][c] u(y), u = cell_unit [648][3], accumulated in fp32 in the order di = -1, 0, 1 outer,
// dj = -1, 0, 1 inner; (az, el) of v in degrees, +180 written as -180; the cell centre when |v|^2 is 0 or not finite.
__device__ __forceinline__ float2 refine_doa(const float* prob, const float* __restrict__ cell_unit, int x, int c) {
  const int i = x / kJ, j = x - i * kJ;
  float vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll
  for (int di = -1; di <= 1; ++di) {
    const int ii = i + di;
    if (ii < 0 || ii >= kI) continue;                  // no wrap over the poles
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      int jj = j + dj;
      jj = jj < 0 ? jj + kJ : (jj >= kJ ? jj - kJ : jj);           // azimuth wraps
      const int y = ii * kJ + jj;
      const float p = prob[y * kC + c];
      vx = fmaf(p, cell_unit[3 * y], vx);
      vy = fmaf(p, cell_unit[3 * y + 1], vy);
      vz = fmaf(p, cell_unit[3 * y + 2], vz);
    }
  }
  const float n2 = vx * vx + vy * vy + vz * vz;
  if (!(n2 > 0.0f) || !(n2 <= 3.0e38f))                // zero, NaN or infinite: the cell centre (exact in fp32)
    return make_float2(-180.0f + (j + 0.5f) * (360.0f / kJ), -90.0f + (i + 0.5f) * (180.0f / kI));
  constexpr float kDeg = 57.295779513082323f;
  float az = atan2f(vy, vx) * kDeg;
  const float el = atan2f(vz, sqrtf(vx * vx + vy * vy)) * kDeg;
  az = az >= 180.0f ? -180.0f : az;
  return make_float2(az, el);
}

// One workgroup's work: meta-frame q0 + blockIdx.x from `logits`; the kernel's only LDS is the staged row declared here.
// kTta: `logits` holds n_pat stacks [n_pat][nw][250][648][14] (stack_chunks 16-byte chunks apart), stack n the windows
// gathered with pattern (patterns >> 4 n) & 15; rows are walked in (frame, window, n) ascending order, the thread that
// owns cell x reads the staged row at cell_dest(x), and a frame's sum is divided once by n_w * n_pat.
// kRefine: after a class's top-K, while P_q is still in LDS, lane r of the wave that selected it writes the sub-cell
// DOA of its detection r to det_dir [nq][13][K][2] (0 past the count).
template <bool kBf16, bool kTta, bool kRefine = false>
__device__ __forceinline__ void decode_meta_frame(
    const uint4* logits, long w0, long nw, long W, long total,
    const int64_t* meta_first, const int32_t* meta_len, long q0, float threshold, int K,
    int32_t* det_cell, float* det_score, int32_t* det_count,
    float* probs_out, uint64_t patterns, int n_pat, long stack_chunks, const float* cell_unit = nullptr,
    float* det_dir = nullptr) {
  using R = Row<kBf16>;
  __shared__ uint4 stage[R::kLdsChunks];
  const int tid = threadIdx.x;
  const long q = q0 + blockIdx.x;
  const long first = meta_first[q];
  const int len = meta_len[q];
  // a meta-frame whose windows are not all in this launch writes nothing (the host refuses such a call before it
  // launches; this keeps a direct caller's mistake from reading outside `logits`)
  if (len < 1 || len > 5 || first < 0 || first + len > total || first_window(first) < w0 ||
      last_window(first + len - 1, W) >= w0 + nw)
    return;

  float pacc[kCellsPerThread][kC], facc[kCellsPerThread][kC];
#pragma unroll
  for (int t = 0; t < kCellsPerThread; ++t)
#pragma unroll
    for (int k = 0; k < kC; ++k) pacc[t][k] = facc[t][k] = 0.0f;
  [[maybe_unused]] int ci[kCellsPerThread], cj[kCellsPerThread];
  if constexpr (kTta) {
#pragma unroll
    for (int t = 0; t < kCellsPerThread; ++t) {
      const int cell = tid + t * kThreads;
      ci[t] = cell / kJ;
      cj[t] = cell - ci[t] * kJ;
    }
  }

  // rows in (frame ascending, window ascending[, stack ascending]) order; the next row's 16-byte loads are in flight
  // while this one is reduced from LDS
  long f = first, w = first_window(first);
  [[maybe_unused]] int n = 0;
  u32x4 next[R::kPerThread];
  load_row<kBf16>(logits, w0, f, w, tid, next);
  const long f_end = first + len;
  while (f < f_end) {
    __syncthreads();                                   // the previous row's readers are done
#pragma unroll
    for (int e = 0; e < R::kPerThread; ++e) {
      const int ch = tid + e * kThreads;
      if (ch < R::kChunks) reinterpret_cast<u32x4*>(stage)[ch] = next[e];
    }
    __syncthreads();
    const long cur_f = f, cur_w = w;
    const long w_last = last_window(cur_f, W);
    [[maybe_unused]] int pattern = 0;
    [[maybe_unused]] bool last_stack = true;
    if constexpr (kTta) {
      pattern = static_cast<int>(patterns >> (4 * n)) & 15;
      last_stack = n + 1 == n_pat;
      n = last_stack ? 0 : n + 1;
    }
    if (last_stack) {
      if (w < w_last) {
        ++w;
      } else {
        ++f;
        if (f < f_end) w = first_window(f);
      }
    }
    if (f < f_end) {
      if constexpr (kTta)
        load_row<kBf16>(logits + n * stack_chunks, w0, f, w, tid, next);
      else
        load_row<kBf16>(logits, w0, f, w, tid, next);
    }
#pragma unroll
    for (int t = 0; t < kCellsPerThread; ++t) {
      const int cell = tid + t * kThreads;
      if (cell < kCells) {
        float p[kC];
        if constexpr (kTta)
          cell_softmax<kBf16>(stage, cell_dest(ci[t], cj[t], pattern), p);
        else
          cell_softmax<kBf16>(stage, cell, p);
#pragma unroll
        for (int k = 0; k < kC; ++k) facc[t][k] += p[k];
      }
    }
    if (cur_w == w_last && last_stack) {               // frame complete: its mean over the covering windows [and stacks]
      float n_w = static_cast<float>(w_last - first_window(cur_f) + 1);
      if constexpr (kTta) n_w *= static_cast<float>(n_pat);        // exact: at most 5 * 16
#pragma unroll
      for (int t = 0; t < kCellsPerThread; ++t)
#pragma unroll
        for (int k = 0; k < kC; ++k) {
          pacc[t][k] += facc[t][k] / n_w;
          facc[t][k] = 0.0f;
        }
    }
  }

  // P_q = mean over the meta-frame's frames, into LDS as [cell][13]
  __syncthreads();
  float* prob = reinterpret_cast<float*>(stage);
  const float n_f = static_cast<float>(len);
#pragma unroll
  for (int t = 0; t < kCellsPerThread; ++t) {
    const int cell = tid + t * kThreads;
    if (cell < kCells)
#pragma unroll
      for (int k = 0; k < kC; ++k) prob[cell * kC + k] = pacc[t][k] / n_f;
  }
  __syncthreads();
  const long qi = blockIdx.x;
  if (probs_out) {
    float4* dst = reinterpret_cast<float4*>(probs_out + qi * kProbFloats);
    const float4* s4 = reinterpret_cast<const float4*>(prob);
    for (int i = tid; i < kProbFloats / 4; i += kThreads) dst[i] = s4[i];
  }

  // peaks and top-K: wave v takes classes v and v + 8; lane l the cells l + 64 t
  const int wave = tid >> 6, lane = tid & 63;
  constexpr int kSlots = (kCells + 63) / 64;           // 11
  for (int c = wave; c < kC; c += kThreads / 64) {
    uint32_t peaks = 0;
#pragma unroll
    for (int t = 0; t < kSlots; ++t) {
      const int x = lane + 64 * t;
      if (x >= kCells) break;
      const float s = prob[x * kC + c];
      if (!(s >= threshold)) continue;
      const int i = x / kJ, j = x - i * kJ;
      bool peak = true;
#pragma unroll
      for (int di = -1; di <= 1; ++di) {
        const int ii = i + di;
        if (ii < 0 || ii >= kI) continue;              // no wrap over the poles
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
          if (di == 0 && dj == 0) continue;
          const int jj = (j + dj + kJ) % kJ;           // azimuth wraps
          const int y = ii * kJ + jj;
          const float sy = prob[y * kC + c];
          peak = peak && (s > sy || (s == sy && x < y));
        }
      }
      if (peak) peaks |= 1u << t;
    }
    float prev_s = 0.0f;
    int prev_c = kCells;                               // nothing selected yet
    int count = 0;
    [[maybe_unused]] int mine = kCells;                // kRefine: lane r keeps the cell of detection r
    const long out = (qi * kC + c) * K;
    for (int r = 0; r < K; ++r) {
      float best_s = 0.0f;
      int best_c = kCells;
#pragma unroll
      for (int t = 0; t < kSlots; ++t) {
        if (!((peaks >> t) & 1u)) continue;
        const int x = lane + 64 * t;
        const float s = prob[x * kC + c];
        if (prev_c != kCells && !before(prev_s, prev_c, s, x)) continue;   // already taken
        if (before(s, x, best_s, best_c)) {
          best_s = s;
          best_c = x;
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float os = __shfl_xor(best_s, off);
        const int oc = __shfl_xor(best_c, off);
        if (before(os, oc, best_s, best_c)) {
          best_s = os;
          best_c = oc;
        }
      }
      if (best_c == kCells) break;                     // wave-uniform
      if (lane == 0) {
        det_cell[out + r] = best_c;
        det_score[out + r] = best_s;
      }
      if constexpr (kRefine) mine = lane == r ? best_c : mine;
      prev_s = best_s;
      prev_c = best_c;
      ++count;
    }
    if constexpr (kRefine) {
      if (lane < K)
        reinterpret_cast<float2*>(det_dir)[out + lane] =
            lane < count ? refine_doa(prob, cell_unit, mine, c) : make_float2(0.0f, 0.0f);
    }
    if (lane == 0) {
      for (int r = count; r < K; ++r) {
        det_cell[out + r] = -1;
        det_score[out + r] = 0.0f;
      }
      det_count[qi * kC + c] = count;
    }
  }
}

// ---- the host prologue of the three entry points -----------------------------------------------------------------------
// `patterns` [n] -> 4 bits each in *packed, pattern n at bits 4 n.  n must be in 1..16, or 0 with `allow_zero` (the plain
// walk: `patterns` is then NULL, and only then); every pattern in 0..15 and none twice.
inline int pack_patterns(const char* who, const int32_t* patterns, int n, bool allow_zero, uint64_t* packed) {
  const std::string name(who);
  if (n < (allow_zero ? 0 : 1) || n > kMaxPatterns)
    return fail(kErrInvalidArgument, name + (allow_zero ? ": n_patterns must be 0 (the plain walk) or in 1..16"
                                                        : ": n_patterns must be in 1..16"));
  if (allow_zero ? (n == 0) != (patterns == nullptr) : !patterns)
    return fail(kErrInvalidArgument, name + (allow_zero ? ": patterns must be NULL exactly when n_patterns is 0"
                                                        : ": null pointer"));
  unsigned seen = 0;
  *packed = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t p = patterns[i];
    if (p < 0 || p >= kMaxPatterns) return fail(kErrInvalidArgument, name + ": pattern outside 0..15");
    if (seen & (1u << p)) return fail(kErrInvalidArgument, name + ": duplicate pattern");
    seen |= 1u << p;
    *packed |= static_cast<uint64_t>(p) << (4 * i);
  }
  return kOk;
}

enum class Patterns { kNone, kOneOrMore, kAny };      // seld_grid_decode, _tta, _refine

// In this order: the library's state, K, is_bf16, the patterns (pack_patterns, unless kNone), the timeline, the window
// and meta-frame range, with `refine` cell_unit and det_dir, the empty call, the other pointers, the 16-byte alignment of
// logits, probs_out and (refine) det_dir, the launch limit.  A caller launches nothing when the code is not kOk or nq is 0.
inline int check_decode_args(const char* who, const void* logits, int is_bf16, int64_t w0, int64_t nw, int64_t W,
                             int64_t total, const int64_t* meta_first, const int32_t* meta_len, int64_t q0, int64_t nq,
                             Patterns mode, const int32_t* patterns, int n_patterns, uint64_t* packed, int K, bool refine,
                             const float* cell_unit, const int32_t* det_cell, const float* det_score,
                             const int32_t* det_count, const float* det_dir, const float* probs_out) {
  const std::string name(who);
  const auto misaligned = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) != 0; };
  if (!current_state()) return kErrNotInitialised;
  if (K < 1 || K > kMaxK) return fail(kErrInvalidArgument, name + ": K must be in 1..8");
  if (is_bf16 != 0 && is_bf16 != 1) return fail(kErrInvalidArgument, name + ": is_bf16 must be 0 or 1");
  if (mode != Patterns::kNone) {
    const int rc = pack_patterns(who, patterns, n_patterns, mode == Patterns::kAny, packed);
    if (rc != kOk) return rc;
  }
  if (total < 1 || W != (total + kHop - 1) / kHop)
    return fail(kErrInvalidArgument, name + ": W must be ceil(total / 50) for a timeline of total >= 1 frames");
  if (w0 < 0 || nw < 1 || w0 + nw > W || q0 < 0 || nq < 0)
    return fail(kErrInvalidArgument, name + ": bad window or meta-frame range");
  if (refine && (!cell_unit || !det_dir)) return fail(kErrInvalidArgument, name + ": null cell_unit or det_dir");
  if (nq == 0) return kOk;
  if (!logits || !meta_first || !meta_len || !det_cell || !det_score || !det_count)
    return fail(kErrInvalidArgument, name + ": null pointer");
  if (misaligned(logits) || (refine && misaligned(det_dir)) || (probs_out && misaligned(probs_out)))
    return fail(kErrUnsupported, name + (refine ? ": logits, det_dir and probs_out must be 16-byte aligned"
                                                : ": logits and probs_out must be 16-byte aligned"));
  if (nq > 0x7fffffffLL) return fail(kErrUnsupported, name + ": too many meta-frames for one launch");
  return kOk;
}

// One workgroup of kThreads per meta-frame; `kernel` is the instantiation the caller picked.
template <class Kernel, class... Args>
inline int launch_meta_frames(Kernel kernel, int64_t nq, void* stream, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nq)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), args...);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace eval
}  // namespace seld
