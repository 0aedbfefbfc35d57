// Per-window class statistics of the label timeline for gfx950: what class-balanced window
// sampling (seld_balance.py) weighs the training windows by.
//
// SELDDataset.mask_tm is uint16 [total_rows][cells], time-major, bit c of a word = class c active in that cell.  The windows
// of a dataset overlap (250 frames at a hop of 50: every frame lies in five of them), so the reduction is cut in two:
//
//   frame_mask_kernel:    frame_mask[t] = OR over the cells of row t.  Reads the timeline ONCE, in 16-byte chunks; this is
//                         the HBM-bound pass (1296 B in, 2 B out per frame at 648 cells).
//   window_count_kernel:  counts[w][c] = frames of window w whose frame_mask has bit c set.  Reads 2 B per frame and window.
//
// Both are integer work: the results do not depend on the grid.  No atomics, no device-scope fence (the second kernel is a
// second launch), no LDS, no scratch.
//
// frame_mask_kernel: one wavefront per group of kFrameGroup consecutive rows -- kFrameGroup * row bytes of contiguous
// memory.  A row of 81 chunks is one full 64-lane load and a ragged one of 17 lanes.  The ragged lanes are not switched
// off: a lane past the row's end re-reads the row's LAST chunk (OR is idempotent, the address is one the load's other lanes
// fetch anyway), and a row past the timeline's end is the timeline's last row (computed, never stored).  So every load is
// unconditional and in bounds, and all kFrameGroup * tiles of them are issued before the first OR.  Two rows share a 32-bit
// word through the six-step lane butterfly.
#include "seld_common.h"

#include "seld_hip.h"

namespace seld {

constexpr int kFrameGroup = 4;                     // rows per wavefront step (even: two rows per butterfly)
constexpr int kFrameWaves = 4;                     // wavefronts per block of frame_mask_kernel
constexpr int kMaxRowTiles = 4;                    // 64-chunk tiles of a row the unrolled form holds (cells <= 2048)
constexpr int kCountColumns = SELD_BALANCE_COLUMNS;
constexpr int kMaxClasses = SELD_BALANCE_MAX_CLASSES;
static_assert(kFrameGroup % 2 == 0, "rows are reduced in pairs");
static_assert(kMaxClasses + 2 == kCountColumns, "classes, any, frames");

// the 16 bits of every cell of a chunk, OR-ed into the low half
__device__ __forceinline__ unsigned fold_chunk(const uint4 v) {
  const unsigned w = (v.x | v.y) | (v.z | v.w);
  return (w | (w >> 16)) & 0xffffu;
}

// OR over the 64 lanes, in every lane
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v |= static_cast<unsigned>(__shfl_xor(static_cast<int>(v), m, 64));
  return v;
}

// Tiles: 64-chunk tiles per row, (row_chunks + 63) / 64.  groups = ceil(total_rows / kFrameGroup) is 32-bit (host); the
// row offset into the timeline is formed in 64 bits.
template <int Tiles>
__global__ void __launch_bounds__(64 * kFrameWaves)
frame_mask_kernel(const uint4* __restrict__ src, int total_rows, int row_chunks, int groups, uint16_t* __restrict__ frame_mask) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = static_cast<int>(blockIdx.x) * kFrameWaves + (static_cast<int>(threadIdx.x) >> 6);
  const int waves = static_cast<int>(gridDim.x) * kFrameWaves;
  int chunk[Tiles];
#pragma unroll
  for (int k = 0; k < Tiles; ++k) chunk[k] = min(k * 64 + lane, row_chunks - 1);
  for (int g = wave; g < groups; g += waves) {
    const int t0 = g * kFrameGroup;
    uint4 v[kFrameGroup][Tiles];
#pragma unroll
    for (int u = 0; u < kFrameGroup; ++u) {
      const uint4* __restrict__ row = src + static_cast<long>(min(t0 + u, total_rows - 1)) * row_chunks;
#pragma unroll
      for (int k = 0; k < Tiles; ++k) v[u][k] = row[chunk[k]];
    }
    unsigned mine = 0;                             // lane u < kFrameGroup keeps row t0 + u
#pragma unroll
    for (int u = 0; u < kFrameGroup; u += 2) {
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int k = 0; k < Tiles; ++k) {
        lo |= fold_chunk(v[u][k]);
        hi |= fold_chunk(v[u + 1][k]);
      }
      const unsigned both = wave_or(lo | (hi << 16));
      if (lane == u) mine = both & 0xffffu;
      if (lane == u + 1) mine = both >> 16;
    }
    if (lane < kFrameGroup && t0 + lane < total_rows) frame_mask[static_cast<long>(t0) + lane] = static_cast<uint16_t>(mine);
  }
}

// counts int32 [n_windows][16]: one wavefront per window.  A lane takes every 64th frame of the window; bit c of the 64
// words is one ballot, its population count the frames of the step that hold class c.  The sums are wave-uniform; lane c
// stores column c, 64 contiguous bytes per window.
__global__ void __launch_bounds__(64)
window_count_kernel(const uint16_t* __restrict__ frame_mask, long total_rows, int window, long hop, int n_windows,
                    unsigned class_bits, int32_t* __restrict__ counts) {
  const int lane = static_cast<int>(threadIdx.x);
  for (long w = blockIdx.x; w < n_windows; w += gridDim.x) {            // 64-bit: w + gridDim.x may pass 2^31
    const long start = w * hop;                                          // < total_rows (host)
    const long left = total_rows - start;
    const int frames = left < window ? static_cast<int>(left) : window;  // tail windows are short
    int sums[kCountColumns];
#pragma unroll
    for (int c = 0; c < kCountColumns; ++c) sums[c] = 0;
    for (int i0 = 0; i0 < frames; i0 += 64) {
      const int i = i0 + lane;
      const unsigned word = i < frames ? (static_cast<unsigned>(frame_mask[start + i]) & class_bits) : 0u;
#pragma unroll
      for (int c = 0; c < kMaxClasses; ++c) sums[c] += __popcll(__ballot((word >> c) & 1u));
      sums[kMaxClasses] += __popcll(__ballot(word != 0u));
    }
    sums[kMaxClasses + 1] = frames;
    int mine = 0;
#pragma unroll
    for (int c = 0; c < kCountColumns; ++c) mine = lane == c ? sums[c] : mine;
    if (lane < kCountColumns) counts[w * kCountColumns + lane] = mine;
  }
}

constexpr int64_t kInt32Max = (int64_t{1} << 31) - 1;

}  // namespace seld

extern "C" {

int seld_frame_class_mask(const uint16_t* mask, int64_t total_rows, int cells, uint16_t* frame_mask, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!mask || !frame_mask) return fail(kErrInvalidArgument, "seld_frame_class_mask: null pointer");
  if (total_rows < 1) return fail(kErrInvalidArgument, "seld_frame_class_mask: total_rows must be positive");
  if (cells < 1) return fail(kErrInvalidArgument, "seld_frame_class_mask: cells must be positive");
  if (cells % 8 != 0)
    return fail(kErrUnsupported, "seld_frame_class_mask: cells must be a multiple of 8 (a row is read in 16-byte chunks)");
  if (cells > kMaxRowTiles * 64 * 8)
    return fail(kErrUnsupported, "seld_frame_class_mask: more than 2048 cells per row");
  if (reinterpret_cast<uintptr_t>(mask) % 16 != 0)
    return fail(kErrUnsupported, "seld_frame_class_mask: mask must be 16-byte aligned");
  if (total_rows > kInt32Max - kFrameGroup)                            // row indices t0 + u stay 32-bit
    return fail(kErrUnsupported, "seld_frame_class_mask: timeline too long for the 32-bit row index");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int row_chunks = cells / 8;
  const int tiles = (row_chunks + 63) / 64;
  const int rows = static_cast<int>(total_rows);
  const int groups = static_cast<int>((total_rows + kFrameGroup - 1) / kFrameGroup);
  const int64_t want = (static_cast<int64_t>(groups) + kFrameWaves - 1) / kFrameWaves;
  const int64_t cap = static_cast<int64_t>(st->num_cus) * 8;           // 4-wave blocks: up to 8 waves per SIMD
  const dim3 grid(static_cast<unsigned>(want < cap ? want : cap)), block(64 * kFrameWaves);
  const uint4* src = reinterpret_cast<const uint4*>(mask);
  switch (tiles) {
    case 1: hipLaunchKernelGGL(frame_mask_kernel<1>, grid, block, 0, stream, src, rows, row_chunks, groups, frame_mask); break;
    case 2: hipLaunchKernelGGL(frame_mask_kernel<2>, grid, block, 0, stream, src, rows, row_chunks, groups, frame_mask); break;
    case 3: hipLaunchKernelGGL(frame_mask_kernel<3>, grid, block, 0, stream, src, rows, row_chunks, groups, frame_mask); break;
    default: hipLaunchKernelGGL(frame_mask_kernel<4>, grid, block, 0, stream, src, rows, row_chunks, groups, frame_mask); break;
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_window_class_frames(const uint16_t* frame_mask, int64_t total_rows, int64_t window, int64_t hop, int64_t n_windows,
                             int num_classes, int32_t* counts, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!frame_mask || !counts) return fail(kErrInvalidArgument, "seld_window_class_frames: null pointer");
  if (total_rows < 1) return fail(kErrInvalidArgument, "seld_window_class_frames: total_rows must be positive");
  if (window < 1 || hop < 1 || n_windows < 1)
    return fail(kErrInvalidArgument, "seld_window_class_frames: window, hop and n_windows must be positive");
  if (num_classes < 1 || num_classes > kMaxClasses)
    return fail(kErrInvalidArgument, "seld_window_class_frames: num_classes must be 1..14");
  if (n_windows - 1 > (total_rows - 1) / hop)                          // (n_windows - 1) * hop >= total_rows, without the product
    return fail(kErrInvalidArgument, "seld_window_class_frames: the last window starts behind the timeline's end");
  if (window > kInt32Max - 64 || n_windows > kInt32Max)               // the frame step i0 + 64 and the counts stay 32-bit
    return fail(kErrUnsupported, "seld_window_class_frames: window above 2^31 - 65 or n_windows above 2^31 - 1");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int64_t cap = static_cast<int64_t>(st->num_cus) * 32;          // one-wave blocks: up to 8 per SIMD
  const unsigned blocks = static_cast<unsigned>(n_windows < cap ? n_windows : cap);
  hipLaunchKernelGGL(window_count_kernel, dim3(blocks), dim3(64), 0, stream, frame_mask, static_cast<long>(total_rows),
                     static_cast<int>(window), static_cast<long>(hop), static_cast<int>(n_windows),
                     (1u << num_classes) - 1u, counts);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
