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
// kernel has the shape of softmax_mse_kernel (loss.hip) and is built from the same pieces (loss_core.h): 256 cells per block
// staged through LDS, 16-byte global traffic, one cell per thread, the logits tile reused for the gradient, double block
// partials; ce_finish_kernel adds them in a fixed order and divides by W.  No global atomics, no memset, nothing read by the
// host: the four launches can be captured.
#include "loss_core.h"

namespace seld {

constexpr int kCeCountRows = 1024;        // rows of 14 class counts the label pass may write
constexpr int kCeMaskPerThread = 8;       // mask labels: one 16-byte load per thread in the label pass

// workspace: [kLossMaxPartials] double partials | double W (padded to 64 B) | [kCeCountRows][14] unsigned counts
constexpr size_t kCeWeightSumOffset = kLossMaxPartials * sizeof(double);
constexpr size_t kCeCountsOffset = kCeWeightSumOffset + 64;
constexpr size_t kCeWorkspaceBytes = kCeCountsOffset + static_cast<size_t>(kCeCountRows) * kLossClasses * sizeof(unsigned);

// argmax(mask_to_dense(m)): the lowest set class bit; no bit among the 14 -> background (the last class)
__device__ __forceinline__ int mask_target(unsigned m) {
  m &= (1u << kLossClasses) - 1u;
  return m ? __ffs(static_cast<int>(m)) - 1 : kLossClasses - 1;
}

// torch.argmax of one dense label row: the first maximal value
__device__ __forceinline__ int dense_target(const float* __restrict__ yp) {
  float y[kLossClasses];
  read_dense_row(yp, y);
  return first_argmax(y);
}

// ---- pass 1: class counts of the targets, one row per block ---------------------------------------------------------
// Lane c (< 14) of every wave keeps the wave's count of class c (ballot + popcount: no atomics on the way); the four waves
// meet in LDS.  kVector: the mask pointer is 16-byte aligned, so a thread's eight cells are one uint4.
template <bool kMaskLabels, bool kVector>
__global__ __launch_bounds__(kLossBlock) void ce_count_kernel(const uint16_t* __restrict__ mask,
                                                            const float* __restrict__ dense, int n_cells,
                                                            unsigned* __restrict__ counts) {
  constexpr int kPer = kMaskLabels ? kCeMaskPerThread : 1;
  constexpr int kTile = kLossBlock * kPer;
  __shared__ unsigned block_counts[kLossClasses];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < kLossClasses) block_counts[tid] = 0u;
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
      t[0] = cell0 < n_cells ? dense_target(dense + static_cast<long>(cell0) * kLossClasses) : -1;
    }
#pragma unroll
    for (int c = 0; c < kLossClasses; ++c) {
      unsigned n = 0u;
#pragma unroll
      for (int j = 0; j < kPer; ++j) n += static_cast<unsigned>(__popcll(__ballot(t[j] == c)));
      if (lane == c) mine += n;
    }
  }
  if (lane < kLossClasses && mine != 0u) atomicAdd(&block_counts[lane], mine);     // LDS, integer
  __syncthreads();
  if (tid < kLossClasses) counts[blockIdx.x * kLossClasses + tid] = block_counts[tid];
}

// ---- pass 2: W = sum_c double(w_c) count_c (class order); no weights: W = n_cells and no count rows are read ------------
__global__ __launch_bounds__(256) void ce_weight_sum_kernel(const unsigned* __restrict__ counts, int rows,
                                                            const float* __restrict__ weights, int n_cells,
                                                            double* __restrict__ weight_sum, float* __restrict__ out) {
  __shared__ unsigned long long part[16][16];
  __shared__ double weighted[kLossClasses];
  const int c = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  unsigned long long s = 0ull;
  if (weights != nullptr && c < kLossClasses) {
    for (int r = r0; r < rows; r += 16 * 8) {        // eight independent loads in flight: the block is latency bound
      unsigned v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = r + 16 * u < rows ? counts[(r + 16 * u) * kLossClasses + c] : 0u;
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
  }
  part[r0][c] = s;
  __syncthreads();
  if (weights != nullptr && threadIdx.x < kLossClasses) {
    unsigned long long n = 0ull;
    for (int r = 0; r < 16; ++r) n += part[r][threadIdx.x];
    weighted[threadIdx.x] = static_cast<double>(weights[threadIdx.x]) * static_cast<double>(n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double w_sum = static_cast<double>(n_cells);
    if (weights != nullptr) {
      w_sum = 0.0;
      for (int k = 0; k < kLossClasses; ++k) w_sum += weighted[k];       // class order
    }
    weight_sum[0] = w_sum;
    out[1] = static_cast<float>(w_sum);
  }
}

// ---- pass 3: value partials and gradient -------------------------------------------------------------------------------
// kFocal = false holds no focal arithmetic at all: it is what gamma == 0 runs, so the default result cannot depend on it.
template <bool kBf16, bool kMaskLabels, bool kGrad, bool kFocal>
__global__ __launch_bounds__(kLossBlock) void softmax_ce_kernel(const void* __restrict__ logits_,
                                                              const uint16_t* __restrict__ mask,
                                                              const float* __restrict__ dense, int n_cells,
                                                              const float* __restrict__ weights, float gamma,
                                                              float grad_scale, const double* __restrict__ weight_sum,
                                                              double* __restrict__ partials, void* __restrict__ grad_) {
  constexpr int M = kLossClasses;
  __shared__ __attribute__((aligned(16))) float tile[kLossBlock * M];
  const int tid = threadIdx.x;
  // the 14 weights and W: uniform addresses, read once per block
  float w[M];
#pragma unroll
  for (int c = 0; c < M; ++c) w[c] = weights != nullptr ? weights[c] : 1.0f;
  const float gs = kGrad ? static_cast<float>(static_cast<double>(grad_scale) / weight_sum[0]) : 0.0f;
  const float gamma_m1 = gamma - 1.0f;
  double local[1] = {0.0};
  const int n_tiles = loss_tile_count(n_cells);

  for (int tileno = blockIdx.x; tileno < n_tiles; tileno += gridDim.x) {
    const auto [cell0, cells_here] = loss_tile(n_cells, tileno);
    load_logits_tile<kBf16>(tile, logits_, cell0, cells_here, tid);
    __syncthreads();

    // ---- one cell per thread
    float g[M];
    if (tid < cells_here) {
      float z[M];
      read_cell(tile, tid, z);
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
          local[0] += static_cast<double>(w_t * q_g * (-log_pt));
          f = q_g - gamma * (e_t * inv) * q_gm1 * log_pt;
        } else {
          f = 0.0f;
        }
      } else {
        local[0] += static_cast<double>(w_t * (-log_pt));
      }
      if (kGrad) {
        const float a = gs * w_t * f;
#pragma unroll
        for (int c = 0; c < M; ++c) g[c] = a * (z[c] * inv - (c == t ? 1.0f : 0.0f));
      }
    }
    if (kGrad) {
      __syncthreads();   // everyone has read its logits: reuse the tile for the gradient
      if (tid < cells_here) write_cell(tile, tid, g);
      __syncthreads();
      store_grad_tile<kBf16>(tile, grad_, cell0, cells_here, tid);
    }
    __syncthreads();
  }
  block_sum_to_partials(local, partials);   // the weighted sum
}

// ---- pass 4: fixed-order sum of the block partials, divided by W ------------------------------------------------------------
__global__ __launch_bounds__(256) void ce_finish_kernel(const double* __restrict__ partials, int n,
                                                        const double* __restrict__ weight_sum, float* __restrict__ out) {
  double s[1] = {strided_sum_256(partials, n)};
  tree_sum_256(s);
  if (threadIdx.x == 0) out[0] = static_cast<float>(s[0] / weight_sum[0]);
}

}  // namespace seld

extern "C" {

int64_t seld_softmax_ce_workspace_bytes(void) { return static_cast<int64_t>(seld::kCeWorkspaceBytes); }

int seld_softmax_ce(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                    int64_t n_cells, int num_classes, const float* class_weights, float focal_gamma, float grad_scale,
                    float* out, void* grad, void* workspace, void* stream_) {
  using namespace seld;
  DeviceState* st;
  const int rc = check_class_loss_args("seld_softmax_ce", num_classes, n_cells <= 0 ? "n_cells must be positive" : nullptr,
                                       "n_cells * num_classes", n_cells, logits, out, workspace, mask, dense_labels, &st);
  if (rc != kOk) return rc;
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
    const long per_block = static_cast<long>(kLossBlock) * (mask != nullptr ? kCeMaskPerThread : 1);
    long want = (n_cells + per_block - 1) / per_block;
    if (want > kCeCountRows) want = kCeCountRows;
    rows = static_cast<int>(want);
    if (mask == nullptr)
      hipLaunchKernelGGL((ce_count_kernel<false, false>), dim3(rows), dim3(kLossBlock), 0, stream, mask, dense_labels, n, counts);
    else if (vec)
      hipLaunchKernelGGL((ce_count_kernel<true, true>), dim3(rows), dim3(kLossBlock), 0, stream, mask, dense_labels, n, counts);
    else
      hipLaunchKernelGGL((ce_count_kernel<true, false>), dim3(rows), dim3(kLossBlock), 0, stream, mask, dense_labels, n, counts);
    SELD_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(ce_weight_sum_kernel, dim3(1), dim3(256), 0, stream, counts, rows, class_weights, n, weight_sum, out);
  SELD_HIP_TRY(hipGetLastError());

  // pass 3 + 4
  const unsigned blocks = class_loss_blocks(st, n_cells);
  dispatch_bools([&](auto bf16, auto mask_labels, auto with_grad, auto focal) {
    hipLaunchKernelGGL((softmax_ce_kernel<bf16.value, mask_labels.value, with_grad.value, focal.value>), dim3(blocks),
                       dim3(kLossBlock), 0, stream, logits, mask, dense_labels, n, class_weights, focal_gamma, grad_scale,
                       weight_sum, partials, grad);
  }, logits_is_bf16 != 0, mask != nullptr, grad != nullptr, focal_gamma != 0.0f);
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(256), 0, stream, partials, static_cast<int>(blocks), weight_sum, out);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
