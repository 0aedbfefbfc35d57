// Fused softmax + weighted cross-entropy class loss with an optional focal factor (value and gradient) for gfx950.
//
// Replaces loss.py:27-41 (class_ce_loss: argmax of the labels + nn.CrossEntropyLoss(weight=w)) and its autograd backward.
//
//   t = target of a cell (dense labels: first maximal class; mask m: lowest set bit of m & 0x3fff, background if none)
//   p = softmax(z),  q = sum_{c != t} p_c,  W = sum_cells w_t
//   L = (1/W) sum_cells w_t q^gamma (-log p_t)
//   dL/dz_k = grad_scale (w_t / W) f (p_k - [k = t]),   f = q^gamma - gamma p_t q^(gamma-1) log p_t
//   gamma = 0: f = 1, exactly nn.CrossEntropyLoss(weight=w) (the weighted mean).  A cell with q == 0 contributes nothing.
//
// W is a global sum the gradient of every cell needs, but it depends on the labels only: ce_count_kernel reads the labels
// (2 B per cell for the mask) and leaves one row of 14 integer class counts per block; ce_weight_sum_kernel (one block) adds
// the rows -- integers: any order gives the same sums -- and forms W = sum_c double(w_c) count_c in class order.  The main
// kernel has the shape of softmax_mse_kernel (loss.hip): 256 cells per block staged through LDS, 16-byte global traffic,
// one cell per thread, the logits tile reused for the gradient, double block partials; ce_finish_kernel adds them in a fixed
// order and divides by W.  No global atomics, no memset, nothing read by the host: the four launches can be captured.
#include <hip/hip_bf16.h>

#include "seld_common.h"

namespace seld {

constexpr int kCeBlock = 256;
constexpr int kCeClasses = 14;
constexpr int kCeMaxPartials = 4096;      // double block partials of the main kernel
constexpr int kCeCountRows = 1024;        // rows of 14 class counts the label pass may write
constexpr int kCeMaskPerThread = 8;       // mask labels: one 16-byte load per thread in the label pass

// workspace: [kCeMaxPartials] double partials | double W (padded to 64 B) | [kCeCountRows][14] unsigned counts
constexpr size_t kCeWeightSumOffset = kCeMaxPartials * sizeof(double);
constexpr size_t kCeCountsOffset = kCeWeightSumOffset + 64;
constexpr size_t kCeWorkspaceBytes = kCeCountsOffset + static_cast<size_t>(kCeCountRows) * kCeClasses * sizeof(unsigned);

__device__ __forceinline__ unsigned short ce_bf16_bits(float f) {
  return __bfloat16_as_ushort(__float2bfloat16(f));   // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
}

// argmax(mask_to_dense(m)): the lowest set class bit; no bit among the 14 -> background (the last class)
__device__ __forceinline__ int mask_target(unsigned m) {
  m &= (1u << kCeClasses) - 1u;
  return m ? __ffs(static_cast<int>(m)) - 1 : kCeClasses - 1;
}

// torch.argmax of one dense label row: the first maximal value
__device__ __forceinline__ int dense_target(const float* __restrict__ yp) {
  float y[kCeClasses];
#pragma unroll
  for (int c = 0; c < kCeClasses; c += 2) {
    const float2 v = *reinterpret_cast<const float2*>(yp + c);
    y[c] = v.x;
    y[c + 1] = v.y;
  }
  int t = 0;
  float best = y[0];
#pragma unroll
  for (int c = 1; c < kCeClasses; ++c) {
    if (y[c] > best) {
      best = y[c];
      t = c;
    }
  }
  return t;
}

// ---- pass 1: class counts of the targets, one row per block ---------------------------------------------------------
// Lane c (< 14) of every wave keeps the wave's count of class c (ballot + popcount: no atomics on the way); the four waves
// meet in LDS.  kVector: the mask pointer is 16-byte aligned, so a thread's eight cells are one uint4.
template <bool kMaskLabels, bool kVector>
__global__ __launch_bounds__(kCeBlock) void ce_count_kernel(const uint16_t* __restrict__ mask,
                                                            const float* __restrict__ dense, int n_cells,
                                                            unsigned* __restrict__ counts) {
  constexpr int kPer = kMaskLabels ? kCeMaskPerThread : 1;
  constexpr int kTile = kCeBlock * kPer;
  __shared__ unsigned block_counts[kCeClasses];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < kCeClasses) block_counts[tid] = 0u;
  __syncthreads();
  unsigned mine = 0u;
  const int n_tiles = (n_cells + kTile - 1) / kTile;
  for (int tileno = blockIdx.x; tileno < n_tiles; tileno += gridDim.x) {
    const int cell0 = tileno * kTile + tid * kPer;
    int t[kPer];
    if (kMaskLabels) {
      unsigned short m[kPer];
      if (kVector && cell0 + kPer <= n_cells) {
        const uint4 v = *reinterpret_cast<const uint4*>(mask + cell0);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          m[2 * k] = static_cast<unsigned short>(w[k] & 0xffffu);
          m[2 * k + 1] = static_cast<unsigned short>(w[k] >> 16);
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) t[j] = mask_target(m[j]);
      } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) t[j] = cell0 + j < n_cells ? mask_target(mask[cell0 + j]) : -1;
      }
    } else {
      t[0] = cell0 < n_cells ? dense_target(dense + static_cast<long>(cell0) * kCeClasses) : -1;
    }
#pragma unroll
    for (int c = 0; c < kCeClasses; ++c) {
      unsigned n = 0u;
#pragma unroll
      for (int j = 0; j < kPer; ++j) n += static_cast<unsigned>(__popcll(__ballot(t[j] == c)));
      if (lane == c) mine += n;
    }
  }
  if (lane < kCeClasses && mine != 0u) atomicAdd(&block_counts[lane], mine);     // LDS, integer
  __syncthreads();
  if (tid < kCeClasses) counts[blockIdx.x * kCeClasses + tid] = block_counts[tid];
}

// ---- pass 2: W = sum_c double(w_c) count_c (class order); no weights: W = n_cells and no count rows are read ------------
__global__ __launch_bounds__(256) void ce_weight_sum_kernel(const unsigned* __restrict__ counts, int rows,
                                                            const float* __restrict__ weights, int n_cells,
                                                            double* __restrict__ weight_sum, float* __restrict__ out) {
  __shared__ unsigned long long part[16][16];
  __shared__ double weighted[kCeClasses];
  const int c = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  unsigned long long s = 0ull;
  if (weights != nullptr && c < kCeClasses) {
    for (int r = r0; r < rows; r += 16 * 8) {        // eight independent loads in flight: the block is latency bound
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = r + 16 * u < rows ? counts[(r + 16 * u) * kCeClasses + c] : 0u;
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
  }
  part[r0][c] = s;
  __syncthreads();
  if (weights != nullptr && threadIdx.x < kCeClasses) {
    unsigned long long n = 0ull;
    for (int r = 0; r < 16; ++r) n += part[r][threadIdx.x];
    weighted[threadIdx.x] = static_cast<double>(weights[threadIdx.x]) * static_cast<double>(n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double w_sum = static_cast<double>(n_cells);
    if (weights != nullptr) {
      w_sum = 0.0;
      for (int k = 0; k < kCeClasses; ++k) w_sum += weighted[k];       // class order
    }
    weight_sum[0] = w_sum;
    out[1] = static_cast<float>(w_sum);
  }
}

// ---- the logits tile: global <-> LDS in 16-byte pieces (full tiles), as softmax_mse_kernel moves it ----------------------
template <bool kBf16>
__device__ __forceinline__ void load_logits_tile(float* __restrict__ tile, const void* __restrict__ logits_, int cell0,
                                                 int cells_here, int tid) {
  constexpr int M = kCeClasses;
  const int elems = cells_here * M;
  if (kBf16 && cells_here == kCeBlock) {
    // full tile: 7168 B = 448 sixteen-byte pieces (the tile base is 16-byte aligned: 256 cells x 28 B)
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(logits_) + static_cast<long>(cell0) * M);
    for (int piece = tid; piece < kCeBlock * M / 8; piece += kCeBlock) {
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
    for (int i = tid * 2; i < elems; i += kCeBlock * 2) {   // elems is even (M = 14)
      const unsigned v = *reinterpret_cast<const unsigned*>(src + i);
      tile[i] = __uint_as_float(v << 16);
      tile[i + 1] = __uint_as_float(v & 0xffff0000u);
    }
  } else {
    const float* src = static_cast<const float*>(logits_) + static_cast<long>(cell0) * M;
    if (cells_here == kCeBlock) {                            // 3584 floats from a 16-byte aligned base
      for (int i = tid * 4; i < kCeBlock * M; i += kCeBlock * 4)
        *reinterpret_cast<float4*>(tile + i) = *reinterpret_cast<const float4*>(src + i);
    } else {
      for (int i = tid; i < elems; i += kCeBlock) tile[i] = src[i];
    }
  }
}

template <bool kBf16>
__device__ __forceinline__ void store_grad_tile(const float* __restrict__ tile, void* __restrict__ grad_, int cell0,
                                                int cells_here, int tid) {
  constexpr int M = kCeClasses;
  const int elems = cells_here * M;
  if (kBf16 && cells_here == kCeBlock) {
    uint4* dst = reinterpret_cast<uint4*>(static_cast<unsigned short*>(grad_) + static_cast<long>(cell0) * M);
    for (int piece = tid; piece < kCeBlock * M / 8; piece += kCeBlock) {
      const float4 a = *reinterpret_cast<const float4*>(tile + piece * 8);
      const float4 b = *reinterpret_cast<const float4*>(tile + piece * 8 + 4);
      uint4 v;
      v.x = ce_bf16_bits(a.x) | (static_cast<unsigned>(ce_bf16_bits(a.y)) << 16);
      v.y = ce_bf16_bits(a.z) | (static_cast<unsigned>(ce_bf16_bits(a.w)) << 16);
      v.z = ce_bf16_bits(b.x) | (static_cast<unsigned>(ce_bf16_bits(b.y)) << 16);
      v.w = ce_bf16_bits(b.z) | (static_cast<unsigned>(ce_bf16_bits(b.w)) << 16);
      dst[piece] = v;
    }
  } else if (kBf16) {
    unsigned short* dst = static_cast<unsigned short*>(grad_) + static_cast<long>(cell0) * M;
    for (int i = tid * 2; i < elems; i += kCeBlock * 2) {
      const unsigned lo = ce_bf16_bits(tile[i]);
      const unsigned hi = ce_bf16_bits(tile[i + 1]);
      *reinterpret_cast<unsigned*>(dst + i) = lo | (hi << 16);
    }
  } else {
    float* dst = static_cast<float*>(grad_) + static_cast<long>(cell0) * M;
    if (cells_here == kCeBlock) {
      for (int i = tid * 4; i < kCeBlock * M; i += kCeBlock * 4)
        *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(tile + i);
    } else {
      for (int i = tid; i < elems; i += kCeBlock) dst[i] = tile[i];
    }
  }
}

// ---- pass 3: value partials and gradient -------------------------------------------------------------------------------
// kFocal = false holds no focal arithmetic at all: it is what gamma == 0 runs, so the default result cannot depend on it.
template <bool kBf16, bool kMaskLabels, bool kGrad, bool kFocal>
__global__ __launch_bounds__(kCeBlock) void softmax_ce_kernel(const void* __restrict__ logits_,
                                                              const uint16_t* __restrict__ mask,
                                                              const float* __restrict__ dense, int n_cells,
                                                              const float* __restrict__ weights, float gamma,
                                                              float grad_scale, const double* __restrict__ weight_sum,
                                                              double* __restrict__ partials, void* __restrict__ grad_) {
  constexpr int M = kCeClasses;
  __shared__ __attribute__((aligned(16))) float tile[kCeBlock * M];
  __shared__ double wave_sums[kCeBlock / 64];
  const int tid = threadIdx.x;
  // the 14 weights and W: uniform addresses, read once per block
  float w[M];
#pragma unroll
  for (int c = 0; c < M; ++c) w[c] = weights != nullptr ? weights[c] : 1.0f;
  const float gs = kGrad ? static_cast<float>(static_cast<double>(grad_scale) / weight_sum[0]) : 0.0f;
  const float gamma_m1 = gamma - 1.0f;
  double local = 0.0;
  // 32-bit tile extents on purpose (the host checks n_cells * M < 2^31): see the note in loss.hip on what hipcc made of a
  // uniform 64-bit min() in this kernel shape
  const int n_tiles = (n_cells + kCeBlock - 1) / kCeBlock;

  for (int tileno = blockIdx.x; tileno < n_tiles; tileno += gridDim.x) {
    const int cell0 = tileno * kCeBlock;
    const int cells_here = min(n_cells - cell0, kCeBlock);
    load_logits_tile<kBf16>(tile, logits_, cell0, cells_here, tid);
    __syncthreads();

    // ---- one cell per thread
    float g[M];
    if (tid < cells_here) {
      float z[M];
#pragma unroll
      for (int c = 0; c < M; c += 2) {
        const float2 v = *reinterpret_cast<const float2*>(tile + tid * M + c);
        z[c] = v.x;
        z[c + 1] = v.y;
      }
      const int t = kMaskLabels ? mask_target(mask[cell0 + tid])
                                : dense_target(dense + static_cast<long>(cell0 + tid) * M);
      float zmax = z[0];
#pragma unroll
      for (int c = 1; c < M; ++c) zmax = fmaxf(zmax, z[c]);
      float denom = 0.0f, others = 0.0f, e_t = 0.0f, z_t = 0.0f, w_t = 0.0f;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const bool is_t = c == t;
        z_t = is_t ? z[c] : z_t;
        w_t = is_t ? w[c] : w_t;
        z[c] = __expf(z[c] - zmax);
        denom += z[c];
        e_t = is_t ? z[c] : e_t;
        others += is_t ? 0.0f : z[c];
      }
      const float inv = 1.0f / denom;
      const float log_pt = (z_t - zmax) - __logf(denom);       // finite whatever the logits' spread
      float f = 1.0f;
      if (kFocal) {
        const float q = others * inv;                          // the other classes' probabilities, not 1 - p_t
        if (q > 0.0f) {
          const float q_gm1 = gamma_m1 == 0.0f ? 1.0f : __builtin_amdgcn_exp2f(gamma_m1 * __builtin_amdgcn_logf(q));
          const float q_g = q_gm1 * q;
          local += static_cast<double>(w_t * q_g * (-log_pt));
          f = q_g - gamma * (e_t * inv) * q_gm1 * log_pt;
        } else {
          f = 0.0f;
        }
      } else {
        local += static_cast<double>(w_t * (-log_pt));
      }
      if (kGrad) {
        const float a = gs * w_t * f;
#pragma unroll
        for (int c = 0; c < M; ++c) g[c] = a * (z[c] * inv - (c == t ? 1.0f : 0.0f));
      }
    }
    if (kGrad) {
      __syncthreads();   // everyone has read its logits: reuse the tile for the gradient
      if (tid < cells_here) {
#pragma unroll
        for (int c = 0; c < M; c += 2) *reinterpret_cast<float2*>(tile + tid * M + c) = make_float2(g[c], g[c + 1]);
      }
      __syncthreads();
      store_grad_tile<kBf16>(tile, grad_, cell0, cells_here, tid);
    }
    __syncthreads();
  }

  // ---- deterministic block reduction of the weighted sum (double)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
  if ((tid & 63) == 0) wave_sums[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < kCeBlock / 64; ++k) s += wave_sums[k];
    partials[blockIdx.x] = s;
  }
}

// ---- pass 4: fixed-order sum of the block partials, divided by W (the form of loss_finish_kernel) --------------------------
__global__ __launch_bounds__(256) void ce_finish_kernel(const double* __restrict__ partials, int n,
                                                        const double* __restrict__ weight_sum, float* __restrict__ out) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = static_cast<float>(part[0] / weight_sum[0]);
}

struct CeLaunch {
  unsigned blocks;
  hipStream_t stream;
  const void* logits;
  const uint16_t* mask;
  const float* dense;
  int n_cells;
  const float* weights;
  float gamma, grad_scale;
  const double* weight_sum;
  double* partials;
  void* grad;
};

template <bool kBf16, bool kMaskLabels, bool kGrad, bool kFocal>
static void launch_main(const CeLaunch& a) {
  hipLaunchKernelGGL((softmax_ce_kernel<kBf16, kMaskLabels, kGrad, kFocal>), dim3(a.blocks), dim3(kCeBlock), 0, a.stream,
                     a.logits, a.mask, a.dense, a.n_cells, a.weights, a.gamma, a.grad_scale, a.weight_sum, a.partials,
                     a.grad);
}

template <bool kBf16, bool kMaskLabels, bool kGrad>
static void launch_focal(const CeLaunch& a, bool focal) {
  if (focal) launch_main<kBf16, kMaskLabels, kGrad, true>(a);
  else launch_main<kBf16, kMaskLabels, kGrad, false>(a);
}

template <bool kBf16, bool kMaskLabels>
static void launch_grad(const CeLaunch& a, bool focal) {
  if (a.grad != nullptr) launch_focal<kBf16, kMaskLabels, true>(a, focal);
  else launch_focal<kBf16, kMaskLabels, false>(a, focal);
}

template <bool kBf16>
static void launch_labels(const CeLaunch& a, bool focal) {
  if (a.mask != nullptr) launch_grad<kBf16, true>(a, focal);
  else launch_grad<kBf16, false>(a, focal);
}

}  // namespace seld

extern "C" {

int64_t seld_softmax_ce_workspace_bytes(void) { return static_cast<int64_t>(seld::kCeWorkspaceBytes); }

int seld_softmax_ce(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                    int64_t n_cells, int num_classes, const float* class_weights, float focal_gamma, float grad_scale,
                    float* out, void* grad, void* workspace, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (num_classes != kCeClasses) return fail(kErrUnsupported, "seld_softmax_ce: built for 14 classes (config.py:40)");
  if (n_cells <= 0) return fail(kErrInvalidArgument, "seld_softmax_ce: n_cells must be positive");
  if (n_cells > (2147483647LL - 4096) / num_classes)
    return fail(kErrUnsupported, "seld_softmax_ce: n_cells * num_classes must stay below 2^31 (32-bit tile indexing)");
  if (!logits || !out || !workspace) return fail(kErrInvalidArgument, "seld_softmax_ce: null pointer");
  if ((mask == nullptr) == (dense_labels == nullptr))
    return fail(kErrInvalidArgument, "seld_softmax_ce: pass exactly one of mask / dense_labels");
  if (!(focal_gamma == 0.0f || (focal_gamma >= 1.0f && focal_gamma <= 3.0e38f)))
    return fail(kErrInvalidArgument, "seld_softmax_ce: focal_gamma must be 0 or a finite value >= 1 "
                                     "(q^(gamma-1) is unbounded for 0 < gamma < 1)");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int n = static_cast<int>(n_cells);
  char* ws = static_cast<char*>(workspace);
  double* partials = reinterpret_cast<double*>(ws);
  double* weight_sum = reinterpret_cast<double*>(ws + kCeWeightSumOffset);
  unsigned* counts = reinterpret_cast<unsigned*>(ws + kCeCountsOffset);

  // pass 1 + 2: W from the labels (without weights W = n_cells: no label pass)
  int rows = 0;
  if (class_weights != nullptr) {
    const bool vec = mask != nullptr && reinterpret_cast<uintptr_t>(mask) % 16 == 0;
    const long per_block = static_cast<long>(kCeBlock) * (mask != nullptr ? kCeMaskPerThread : 1);
    long want = (n_cells + per_block - 1) / per_block;
    if (want > kCeCountRows) want = kCeCountRows;
    rows = static_cast<int>(want);
    if (mask == nullptr)
      hipLaunchKernelGGL((ce_count_kernel<false, false>), dim3(rows), dim3(kCeBlock), 0, stream, mask, dense_labels, n, counts);
    else if (vec)
      hipLaunchKernelGGL((ce_count_kernel<true, true>), dim3(rows), dim3(kCeBlock), 0, stream, mask, dense_labels, n, counts);
    else
      hipLaunchKernelGGL((ce_count_kernel<true, false>), dim3(rows), dim3(kCeBlock), 0, stream, mask, dense_labels, n, counts);
    SELD_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ce_weight_sum_kernel, dim3(1), dim3(256), 0, stream, counts, rows, class_weights, n, weight_sum, out);
  SELD_HIP_TRY(hipGetLastError());

  // pass 3 + 4
  long tiles = (n_cells + kCeBlock - 1) / kCeBlock;
  long blocks = static_cast<long>(st->num_cus) * 8;
  if (blocks > tiles) blocks = tiles;
  if (blocks > kCeMaxPartials) blocks = kCeMaxPartials;
  const CeLaunch a{static_cast<unsigned>(blocks), stream, logits, mask, dense_labels, n, class_weights, focal_gamma,
                   grad_scale, weight_sum, partials, grad};
  if (logits_is_bf16) launch_labels<true>(a, focal_gamma != 0.0f);
  else launch_labels<false>(a, focal_gamma != 0.0f);
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, stream, partials, static_cast<int>(blocks), weight_sum, out);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
