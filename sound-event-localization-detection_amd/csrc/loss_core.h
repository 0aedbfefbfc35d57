// What the three fused class losses share (loss.hip, loss_ce.hip, loss3.hip): a 256-thread block stages 256 cells of 14
// logits through LDS so that global traffic is full 16-byte lanes while each thread owns one cell, reuses the tile for the
// gradient, and leaves fixed-order double partials for a one-block finish kernel.  The arithmetic between the cell read and
// the cell write is each kernel's own.
#pragma once

#include <string>
#include <type_traits>

#include "seld_bf16.h"
#include "seld_common.h"

namespace seld {

constexpr int kLossBlock = 256;            // threads per block = cells per tile
constexpr int kLossClasses = 14;           // config.py:40
constexpr int kLossMaxPartials = 4096;     // blocks of a main kernel = double partials per sum

// ---- the tile extent ------------------------------------------------------------------------------------------------------
// All index arithmetic is 32-bit on purpose (the host checks n_cells * 14 < 2^31).  With 64-bit extents hipcc
// (ROCm 7.2, gfx950) emitted, for some instantiations of softmax_mse_kernel, a v_cmp_lt_i64 followed by s_cselect
// WITHOUT copying VCC to SCC for `min(n_cells - cell0, 256)`: the ragged last tile was then processed as a full
// one and read 256 cells of whatever lies behind the logits / labels (wrong sums, NaN, or a memory fault).
// s_min_i32 cannot go wrong that way; tests/test_loss_gpu.py::test_every_variant_at_ragged_sizes covers it.
struct LossTile {
  int cell0, cells_here;
};

__device__ __forceinline__ int loss_tile_count(int n_cells) { return (n_cells + kLossBlock - 1) / kLossBlock; }

__device__ __forceinline__ LossTile loss_tile(int n_cells, int tileno) {
  const int cell0 = tileno * kLossBlock;
  return LossTile{cell0, min(n_cells - cell0, kLossBlock)};
}

// ---- the logits tile: global <-> LDS ---------------------------------------------------------------------------------------
// A full tile (7168 B of bf16, 14336 B of fp32) behind a 16-byte aligned base pointer is itself 16-byte aligned and moves in
// 16-byte pieces; a ragged tile, or any tile of a misaligned tensor, moves element by element (bf16: in pairs, 14 is even).
// The test is wave-uniform, and the load and the store each look at their own pointer.  The element loops run for one tile
// per launch at most (or for a misaligned tensor) and stay rolled (`unroll 1`): unrolled, their hoisted addresses live
// across the whole tile loop and cost several instantiations an occupancy step (compiler resource report, ROCm 7.2).
//
// One comparison per tile, against a size no tile has when the base is misaligned.  Written as two tests
// (`cells_here == 256 && aligned`) the focal gradient instantiations of softmax_ce_kernel took 101 instead of 97 SGPRs,
// one more than eight waves per SIMD allow.
__device__ __forceinline__ bool full_aligned_tile(const void* base, int cells_here) {
  const int vector_cells = (reinterpret_cast<uintptr_t>(base) & 15u) == 0 ? kLossBlock : 0;
  return cells_here == vector_cells;
}

template <bool kBf16>
__device__ __forceinline__ void load_logits_tile(float* __restrict__ tile, const void* __restrict__ logits_, int cell0,
                                                 int cells_here, int tid) {
  constexpr int M = kLossClasses;
  const int elems = cells_here * M;
  const bool fast = full_aligned_tile(logits_, cells_here);
  if (kBf16 && fast) {
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(logits_) + static_cast<long>(cell0) * M);
    for (int piece = tid; piece < kLossBlock * M / 8; piece += kLossBlock) {
      const uint4 v = src[piece];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      float f[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        f[2 * k] = __uint_as_float(w[k] << 16);
        f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
      }
      *reinterpret_cast<float4*>(tile + piece * 8) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<float4*>(tile + piece * 8 + 4) = make_float4(f[4], f[5], f[6], f[7]);
    }
  } else if (kBf16) {
    const unsigned short* src = static_cast<const unsigned short*>(logits_) + static_cast<long>(cell0) * M;
#pragma unroll 1
    for (int i = tid * 2; i < elems; i += kLossBlock * 2) {
      const unsigned v = *reinterpret_cast<const unsigned*>(src + i);
      tile[i] = __uint_as_float(v << 16);
      tile[i + 1] = __uint_as_float(v & 0xffff0000u);
    }
  } else {
    const float* src = static_cast<const float*>(logits_) + static_cast<long>(cell0) * M;
    if (fast) {
      for (int i = tid * 4; i < kLossBlock * M; i += kLossBlock * 4)
        *reinterpret_cast<float4*>(tile + i) = *reinterpret_cast<const float4*>(src + i);
    } else {
#pragma unroll 1
      for (int i = tid; i < elems; i += kLossBlock) tile[i] = src[i];
    }
  }
}

template <bool kBf16>
__device__ __forceinline__ void store_grad_tile(const float* __restrict__ tile, void* __restrict__ grad_, int cell0,
                                                int cells_here, int tid) {
  constexpr int M = kLossClasses;
  const int elems = cells_here * M;
  const bool fast = full_aligned_tile(grad_, cells_here);
  if (kBf16 && fast) {
    uint4* dst = reinterpret_cast<uint4*>(static_cast<unsigned short*>(grad_) + static_cast<long>(cell0) * M);
    for (int piece = tid; piece < kLossBlock * M / 8; piece += kLossBlock) {
      const float4 a = *reinterpret_cast<const float4*>(tile + piece * 8);
      const float4 b = *reinterpret_cast<const float4*>(tile + piece * 8 + 4);
      dst[piece] = make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
    }
  } else if (kBf16) {
    unsigned short* dst = static_cast<unsigned short*>(grad_) + static_cast<long>(cell0) * M;
#pragma unroll 1
    for (int i = tid * 2; i < elems; i += kLossBlock * 2)
      *reinterpret_cast<unsigned*>(dst + i) = pack_bf16x2(tile[i], tile[i + 1]);
  } else {
    float* dst = static_cast<float*>(grad_) + static_cast<long>(cell0) * M;
    if (fast) {
      for (int i = tid * 4; i < kLossBlock * M; i += kLossBlock * 4)
        *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(tile + i);
    } else {
#pragma unroll 1
      for (int i = tid; i < elems; i += kLossBlock) dst[i] = tile[i];
    }
  }
}

// ---- one cell per thread ---------------------------------------------------------------------------------------------------
// stride-14 LDS accesses as 7 x ds_read_b64 / ds_write_b64: conflict free
__device__ __forceinline__ void read_cell(const float* tile, int tid, float (&z)[kLossClasses]) {
#pragma unroll
  for (int c = 0; c < kLossClasses; c += 2) {
    const float2 v = *reinterpret_cast<const float2*>(tile + tid * kLossClasses + c);
    z[c] = v.x;
    z[c + 1] = v.y;
  }
}

__device__ __forceinline__ void write_cell(float* tile, int tid, const float (&g)[kLossClasses]) {
#pragma unroll
  for (int c = 0; c < kLossClasses; c += 2)
    *reinterpret_cast<float2*>(tile + tid * kLossClasses + c) = make_float2(g[c], g[c + 1]);
}

// the multi-hot row of a class mask; no bit at all means background (the last class), dataset.py:114-117
__device__ __forceinline__ void mask_to_one_hot(unsigned m, float (&y)[kLossClasses]) {
#pragma unroll
  for (int c = 0; c < kLossClasses; ++c) y[c] = ((m >> c) & 1u) ? 1.0f : 0.0f;
  if (m == 0u) y[kLossClasses - 1] = 1.0f;
}

// one row of dense labels
__device__ __forceinline__ void read_dense_row(const float* __restrict__ yp, float (&y)[kLossClasses]) {
#pragma unroll
  for (int c = 0; c < kLossClasses; c += 2) {
    const float2 v = *reinterpret_cast<const float2*>(yp + c);
    y[c] = v.x;
    y[c + 1] = v.y;
  }
}

// torch.argmax of one row: the first maximal value
__device__ __forceinline__ int first_argmax(const float (&y)[kLossClasses]) {
  int t = 0;
  float best = y[0];
#pragma unroll
  for (int c = 1; c < kLossClasses; ++c) {
    if (y[c] > best) {
      best = y[c];
      t = c;
    }
  }
  return t;
}

// z <- exp(z - max z); returns 1 / sum.  softmax_ce_kernel picks its target's terms between these exponentials and keeps
// its own loop -- and its own max: taken from a helper it costs that kernel four VGPRs and, in one instantiation, an
// occupancy step.
__device__ __forceinline__ float softmax_front(float (&z)[kLossClasses]) {
  float zmax = z[0];
#pragma unroll
  for (int c = 1; c < kLossClasses; ++c) zmax = fmaxf(zmax, z[c]);
  float denom = 0.0f;
#pragma unroll
  for (int c = 0; c < kLossClasses; ++c) {
    z[c] = __expf(z[c] - zmax);
    denom += z[c];
  }
  return 1.0f / denom;
}

// ---- deterministic sums (double) -------------------------------------------------------------------------------------------
// K per-thread sums of a main kernel -> partials[k * gridDim.x + blockIdx.x]: wave shuffle, then the four waves in order.
template <int K>
__device__ __forceinline__ void block_sum_to_partials(double (&local)[K], double* __restrict__ partials) {
  __shared__ double wave_sums[K][kLossBlock / 64];
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < K; ++k) local[k] += __shfl_down(local[k], off, 64);
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) wave_sums[k][tid >> 6] = local[k];
  __syncthreads();
  if (tid < K) {
    double s = 0.0;
    for (int w = 0; w < kLossBlock / 64; ++w) s += wave_sums[tid][w];
    partials[tid * gridDim.x + blockIdx.x] = s;
  }
}

// a finish kernel's (one block of 256) strided share of n values
__device__ __forceinline__ double strided_sum_256(const double* __restrict__ v, int n) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  return s;
}

// fixed 256-lane tree over K per-thread sums; every thread returns with the totals in s
template <int K>
__device__ __forceinline__ void tree_sum_256(double (&s)[K]) {
  __shared__ double part[K][256];
  for (int k = 0; k < K; ++k) part[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off)
      for (int k = 0; k < K; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + off];
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) s[k] = part[k][0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The refusals the three entry points share, in their order; `name` prefixes every message.  `shape_error` is the entry
// point's own verdict on its extents (null: fine), `product` is what it calls the quantity that must stay below 2^31.
inline int check_class_loss_args(const char* name, int num_classes, const char* shape_error, const char* product,
                                 int64_t n_cells, const void* logits, const void* out, const void* workspace,
                                 const void* mask, const void* dense_labels, DeviceState** st) {
  *st = current_state();
  if (!*st) return kErrNotInitialised;
  const std::string who = std::string(name) + ": ";
  if (num_classes != kLossClasses) return fail(kErrUnsupported, who + "built for 14 classes (config.py:40)");
  if (shape_error) return fail(kErrInvalidArgument, who + shape_error);
  if (n_cells > (2147483647LL - 4096) / num_classes)
    return fail(kErrUnsupported, who + product + " must stay below 2^31 (32-bit tile indexing)");
  if (!logits || !out || !workspace) return fail(kErrInvalidArgument, who + "null pointer");
  if ((mask == nullptr) == (dense_labels == nullptr))
    return fail(kErrInvalidArgument, who + "pass exactly one of mask / dense_labels");
  return kOk;
}

// blocks of a main kernel: eight per CU, no more than there are tiles or partials
inline unsigned class_loss_blocks(const DeviceState* st, int64_t n_cells) {
  long tiles = (n_cells + kLossBlock - 1) / kLossBlock;
  long blocks = static_cast<long>(st->num_cus) * 8;
  if (blocks > tiles) blocks = tiles;
  if (blocks > kLossMaxPartials) blocks = kLossMaxPartials;
  return static_cast<unsigned>(blocks);
}

// runtime booleans -> template arguments: f(std::true_type / std::false_type ...), one per boolean, in order
template <class F>
void dispatch_bools(F&& f) {
  f();
}

template <class F, class... Rest>
void dispatch_bools(F&& f, bool b, Rest... rest) {
  if (b) dispatch_bools([&](auto... tail) { f(std::true_type{}, tail...); }, rest...);
  else dispatch_bools([&](auto... tail) { f(std::false_type{}, tail...); }, rest...);
}

}  // namespace seld
