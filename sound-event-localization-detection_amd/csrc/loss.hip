// Fused softmax + MSE class loss (forward value and gradient in one pass) for gfx950.
//
// Replaces loss.py:43-54 (class_mse_loss: F.softmax + F.mse_loss over [B,T,648,14]) and its
// autograd backward: unfused that is >= 6 passes over 9.07 MB-per-window tensors plus a dense
// 290 MB/step label upload; here the logits are read once, the gradient written once, and the
// labels come either as the dense float tensor the reference uses or as the compact uint16
// class mask (labels.hip), expanded in registers.
//
//   p = softmax(z),  L = mean_{cells,classes} (p - y)^2
//   dL/dz_k = (2/(n*M)) * p_k * [ (p_k - y_k) - sum_c p_c (p_c - y_c) ]
//
// HBM-bound: 56 B read + 56 B written per cell (fp32 logits, M = 14).  A 256-thread block
// stages 256 cells (3584 floats) through LDS so that global traffic is full 16-B lanes while
// each thread owns one cell (stride-14 LDS reads as 7 x ds_read_b64: conflict free).  The tile
// mover, the cell softmax and the block sum are loss_core.h's, shared with loss_ce.hip and loss3.hip.
#include "loss_core.h"

namespace seld {

template <int M, bool kBf16, bool kMaskLabels, bool kGrad>
__global__ __launch_bounds__(kLossBlock) void softmax_mse_kernel(const void* __restrict__ logits_,
                                                                  const uint16_t* __restrict__ mask,
                                                                  const float* __restrict__ dense,
                                                                  int n_cells, float grad_scale,
                                                                  double* __restrict__ partials,
                                                                  void* __restrict__ grad_) {
  static_assert(M == kLossClasses, "the tile helpers of loss_core.h are built for 14 classes");
  __shared__ __attribute__((aligned(16))) float tile[kLossBlock * M];
  const int tid = threadIdx.x;
  double local[1] = {0.0};
  const int n_tiles = loss_tile_count(n_cells);

  for (int tileno = blockIdx.x; tileno < n_tiles; tileno += gridDim.x) {
    const auto [cell0, cells_here] = loss_tile(n_cells, tileno);
    load_logits_tile<kBf16>(tile, logits_, cell0, cells_here, tid);
    __syncthreads();

    // ---- one cell per thread
    float g[M];
    if (tid < cells_here) {
      float z[M], y[M];
      read_cell(tile, tid, z);
      if (kMaskLabels) {
        mask_to_one_hot(mask[cell0 + tid], y);
      } else {
        read_dense_row(dense + static_cast<long>(cell0 + tid) * M, y);
      }
      const float inv = softmax_front(z);
      float sq = 0.0f, dot = 0.0f;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const float p = z[c] * inv;
        const float d = p - y[c];
        sq = fmaf(d, d, sq);
        dot = fmaf(p, d, dot);
        z[c] = p;
        y[c] = d;
      }
      local[0] += static_cast<double>(sq);
      if (kGrad) {
#pragma unroll
        for (int c = 0; c < M; ++c) g[c] = grad_scale * z[c] * (y[c] - dot);
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
  block_sum_to_partials(local, partials);   // the squared-error sum
}

// Fixed-order final reduction -> mean squared error as float.
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ partials, int n, double inv_count,
                                                          float* __restrict__ out) {
  double s[1] = {strided_sum_256(partials, n)};
  tree_sum_256(s);
  if (threadIdx.x == 0) out[0] = static_cast<float>(s[0] * inv_count);
}

// grad *= *scale, where the scale is a DEVICE scalar (the upstream gradient of the loss, known only to the stream).
// loss.backward() hands the loss an upstream gradient of exactly 1: every block then returns after one load and the
// 145 MB gradient is not touched again -- without the host ever reading the scalar.
template <bool kBf16>
__global__ __launch_bounds__(256) void scale_by_scalar_kernel(void* __restrict__ data, long n8,
                                                              const float* __restrict__ scale) {
  const float s = *scale;
  if (s == 1.0f) return;
  for (long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x; i < n8; i += static_cast<long>(gridDim.x) * 256) {
    if (kBf16) {
      uint4 v = static_cast<uint4*>(data)[i];
      unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float lo = __uint_as_float(w[k] << 16) * s, hi = __uint_as_float(w[k] & 0xffff0000u) * s;
        w[k] = pack_bf16x2(lo, hi);
      }
      static_cast<uint4*>(data)[i] = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      float4* p = static_cast<float4*>(data) + 2 * i;
      float4 a = p[0], b = p[1];
      a.x *= s; a.y *= s; a.z *= s; a.w *= s;
      b.x *= s; b.y *= s; b.z *= s; b.w *= s;
      p[0] = a;
      p[1] = b;
    }
  }
}

}  // namespace seld

extern "C" {

int64_t seld_softmax_mse_workspace_bytes(void) { return seld::kLossMaxPartials * sizeof(double); }

int seld_scale_by_device_scalar(void* data, int is_bf16, int64_t n, const float* scale, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (n < 0 || n % 8 != 0) return fail(kErrInvalidArgument, "seld_scale_by_device_scalar: n must be a multiple of 8");
  if (n == 0) return kOk;
  if (!data || !scale) return fail(kErrInvalidArgument, "seld_scale_by_device_scalar: null pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long n8 = n / 8;
  long blocks = (n8 + 255) / 256;
  const long cap = static_cast<long>(st->num_cus > 0 ? st->num_cus : 256) * 8;
  if (blocks > cap) blocks = cap;
  if (is_bf16) hipLaunchKernelGGL(scale_by_scalar_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                                  stream, data, n8, scale);
  else hipLaunchKernelGGL(scale_by_scalar_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream,
                          data, n8, scale);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_softmax_mse(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                     int64_t n_cells, int num_classes, float grad_scale, float* loss_out, void* grad,
                     void* workspace, void* stream_) {
  using namespace seld;
  DeviceState* st;
  const int rc = check_class_loss_args("seld_softmax_mse", num_classes, n_cells <= 0 ? "n_cells must be positive" : nullptr,
                                       "n_cells * num_classes", n_cells, logits, loss_out, workspace, mask, dense_labels, &st);
  if (rc != kOk) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned blocks = class_loss_blocks(st, n_cells);
  double* partials = static_cast<double*>(workspace);
  const int n = static_cast<int>(n_cells);
  dispatch_bools([&](auto bf16, auto mask_labels, auto with_grad) {
    hipLaunchKernelGGL((softmax_mse_kernel<kLossClasses, bf16.value, mask_labels.value, with_grad.value>), dim3(blocks),
                       dim3(kLossBlock), 0, stream, logits, mask, dense_labels, n, grad_scale, partials, grad);
  }, logits_is_bf16 != 0, mask != nullptr, grad != nullptr);
  SELD_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, stream, partials, static_cast<int>(blocks),
                     1.0 / (static_cast<double>(n_cells) * num_classes), loss_out);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
