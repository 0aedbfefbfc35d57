// The three-term SMR-SELD loss of smrl_seld_gaussian.py:946-1072 (= loss.py:43-54, 56-146 applied to probabilities),
// value and gradient in ONE pass over the logits, for gfx950:
//
//   total = w_class * MSE(softmax(z), y) + w_aiur * AIUR + w_cl * CL
//
//   MSE  : mean over all (cell, class) of (p - y)^2                                    smrl_seld_gaussian.py:959-962
//   AIUR : 1 - mean over frames of |pred events AND true events| / |pred OR true|, events = argmax != background,
//          frames without any event on either side count as IoU 1; argmax based, no gradient       :964-997
//   CL   : sum over frames WITH events and cells of  pred_nonbg * y_at  / (frames_with_events * I * J + 1e-10),
//          pred_nonbg = 1 - p_background, y' = 1 on background cells and -N_bac / (N_non + 1e-10) on event cells,
//          y_at = y' + mean over the 8 circular neighbours of (y'_nb - y') = the MEAN OF THE 8 NEIGHBOURS' y'  :999-1055
//
// Two kernels.  `cl_prepare_kernel` reads only the labels (one block per frame): event flags, N_non / N_bac, the
// attention map y_at (zero on frames without events), the frame's true-event count and the number of frames with events.
// `smr_loss_kernel` is the softmax-MSE kernel of loss.hip (one cell per thread, 256-cell tiles staged through LDS: the
// pieces of loss_core.h) with two additions per cell: the CL term and its gradient through the softmax,
//     d CL / d z_k = c * p_k * p_bg (k != bg),   d CL / d z_bg = -c * p_bg * (1 - p_bg),   c = w_cl * y_at / denom,
// and the predicted-event flag, counted per frame with one integer atomic per (block, frame) -- integer sums are
// order independent, so the result is deterministic; the value sums use fixed-order double partials like loss.hip.
// HBM-bound like loss.hip: + 4 B per cell of attention map.
#include "loss_core.h"

namespace seld {

namespace {

constexpr int kL3MaxCells = 1024;          // grid cells per frame the prepare kernel holds in LDS (18 x 36 = 648)

struct Loss3Args {
  const void* logits;          // [n_cells][14] fp32 / bf16
  const uint16_t* mask;        // [n_cells] or null
  const float* dense;          // [n_cells][14] or null
  const float* att;            // [n_cells] attention map (0 on frames without events)
  const int* frames_with_events;   // device scalar
  int* frame_counts;           // [frames][2]: predicted events, intersection with true events (zeroed by prepare)
  int n_cells, cells_per_frame;
  float mse_grad_scale;        // w_class * 2 / (n_cells * 14), or 0 with grad == null
  float w_cl;
  double* partials;            // [2][blocks]: squared error, CL numerator
  void* grad;                  // like logits, or null
};

template <bool kMask>
__global__ __launch_bounds__(kLossBlock) void cl_prepare_kernel(const uint16_t* __restrict__ mask,
                                                              const float* __restrict__ dense, int rows, int cols,
                                                              float* __restrict__ att, int* __restrict__ true_count,
                                                              int* __restrict__ frame_counts,
                                                              int* __restrict__ frames_with_events) {
  __shared__ float yprime[kL3MaxCells];
  __shared__ int counts[3];                 // event cells (CL), background cells (CL), argmax events (AIUR)
  const int frame = blockIdx.x, cells = rows * cols, tid = threadIdx.x;
  if (tid < 3) counts[tid] = 0;
  __syncthreads();
  int n_non = 0, n_bac = 0, n_arg = 0;
  for (int cell = tid; cell < cells; cell += kLossBlock) {
    float nonbg;
    bool arg_event;
    if (kMask) {
      const unsigned m = mask[static_cast<long>(frame) * cells + cell];
      nonbg = static_cast<float>(__popc(m & 0x1fffu));          // sum of the 13 event classes of the multi-hot row
      arg_event = (m & 0x1fffu) != 0u;                          // first maximum of the row is an event class
    } else {
      const float* y = dense + (static_cast<long>(frame) * cells + cell) * kLossClasses;
      nonbg = 0.0f;
      int best = 0;
      float top = y[0];
#pragma unroll
      for (int c = 0; c < kLossClasses; ++c) {
        const float v = y[c];
        if (c < kLossClasses - 1) nonbg += v;
        if (v > top) { top = v; best = c; }
      }
      arg_event = best != kLossClasses - 1;
    }
    const bool event = nonbg > 0.01f;
    n_non += event ? 1 : 0;
    n_bac += nonbg < 0.01f ? 1 : 0;
    n_arg += arg_event ? 1 : 0;
    yprime[cell] = event ? -1.0f : 1.0f;                        // event cells get their value after the counts
  }
  atomicAdd(&counts[0], n_non);
  atomicAdd(&counts[1], n_bac);
  atomicAdd(&counts[2], n_arg);
  __syncthreads();
  const int non = counts[0];
  const float ratio = -(static_cast<float>(counts[1]) / (static_cast<float>(non) + 1e-10f));
  for (int cell = tid; cell < cells; cell += kLossBlock)
    if (yprime[cell] < 0.0f) yprime[cell] = ratio;
  __syncthreads();
  for (int cell = tid; cell < cells; cell += kLossBlock) {
    const int i = cell / cols, j = cell - i * cols;
    float sum = 0.0f;
    // the reference's order of the eight additions (di outer, dj inner), each term (neighbour - centre)
    const float centre = yprime[cell];
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        if (di == 0 && dj == 0) continue;
        const int ii = (i + di + rows) % rows, jj = (j + dj + cols) % cols;
        sum += yprime[ii * cols + jj] - centre;
      }
    att[static_cast<long>(frame) * cells + cell] = non > 0 ? centre + sum / 8.0f : 0.0f;
  }
  if (tid == 0) {
    true_count[frame] = counts[2];
    frame_counts[2 * frame] = 0;
    frame_counts[2 * frame + 1] = 0;
    if (non > 0) atomicAdd(frames_with_events, 1);
  }
}

template <bool kBf16, bool kMask, bool kGrad>
__global__ __launch_bounds__(kLossBlock) void smr_loss_kernel(const Loss3Args a) {
  __shared__ __attribute__((aligned(16))) float tile[kLossBlock * kLossClasses];
  __shared__ int seg_counts[2][2];           // [frame segment of the tile][pred, inter]
  const int tid = threadIdx.x;
  double local[2] = {0.0, 0.0};              // squared error, CL numerator
  const int n_tiles = loss_tile_count(a.n_cells);
  const float cl_scale = a.w_cl / (static_cast<float>(*a.frames_with_events) * static_cast<float>(a.cells_per_frame) + 1e-10f);

  for (int tileno = blockIdx.x; tileno < n_tiles; tileno += gridDim.x) {
    const auto [cell0, cells_here] = loss_tile(a.n_cells, tileno);
    if (tid < 4) seg_counts[tid >> 1][tid & 1] = 0;
    load_logits_tile<kBf16>(tile, a.logits, cell0, cells_here, tid);
    __syncthreads();

    const int first_frame = cell0 / a.cells_per_frame;
    float g[kLossClasses];
    if (tid < cells_here) {
      const int cell = cell0 + tid;
      float z[kLossClasses], y[kLossClasses];
      read_cell(tile, tid, z);
      bool true_event;
      if (kMask) {
        const unsigned m = a.mask[cell];
        mask_to_one_hot(m, y);
        true_event = (m & 0x1fffu) != 0u;
      } else {
        read_dense_row(a.dense + static_cast<long>(cell) * kLossClasses, y);
        true_event = first_argmax(y) != kLossClasses - 1;
      }
      const float inv = softmax_front(z);
      float sq = 0.0f, dot = 0.0f;
      int best = 0;
      float top = -1.0f;
#pragma unroll
      for (int c = 0; c < kLossClasses; ++c) {
        const float p = z[c] * inv;
        if (p > top) { top = p; best = c; }                      // first maximum, like torch.argmax on the probabilities
        const float d = p - y[c];
        sq = fmaf(d, d, sq);
        dot = fmaf(p, d, dot);
        z[c] = p;
        y[c] = d;
      }
      local[0] += static_cast<double>(sq);
      const float p_bg = z[kLossClasses - 1];
      const float w = a.att[cell];
      float pred_nonbg;
      {
        // p_bg is the product z_bg * (1 / denom): left to the compiler, `1 - p_bg` becomes a subtraction in some
        // instantiations and a fused multiply-add in others, and the value-only and the gradient kernels (and the
        // mask and the dense ones) stop agreeing in the last bit.  Always the subtraction.
#pragma clang fp contract(off)
        pred_nonbg = 1.0f - p_bg;
      }
      local[1] += static_cast<double>(pred_nonbg * w);
      if (best != kLossClasses - 1) {                                    // a predicted event: per-frame counts for the AIUR
        const int frame = cell / a.cells_per_frame;
        if (a.cells_per_frame >= kLossBlock) {                     // a 256-cell tile then spans <= 2 frames: count in LDS
          atomicAdd(&seg_counts[frame - first_frame][0], 1);
          if (true_event) atomicAdd(&seg_counts[frame - first_frame][1], 1);
        } else {                                                 // toy grids: straight to the frame's counters
          atomicAdd(&a.frame_counts[2 * frame], 1);
          if (true_event) atomicAdd(&a.frame_counts[2 * frame + 1], 1);
        }
      }
      if (kGrad) {
        const float c_cl = cl_scale * w * p_bg;
#pragma unroll
        for (int c = 0; c < kLossClasses - 1; ++c) g[c] = fmaf(a.mse_grad_scale * z[c], y[c] - dot, c_cl * z[c]);
        g[kLossClasses - 1] = fmaf(a.mse_grad_scale * p_bg, y[kLossClasses - 1] - dot, -c_cl * pred_nonbg);
      }
    }
    __syncthreads();                                             // logits consumed, segment counts complete
    if (tid < 4) {
      const int v = seg_counts[tid >> 1][tid & 1];
      const int frame = first_frame + (tid >> 1);
      if (v != 0 && static_cast<long>(frame) * a.cells_per_frame < a.n_cells) atomicAdd(&a.frame_counts[2 * frame + (tid & 1)], v);
    }
    if (kGrad) {
      if (tid < cells_here) write_cell(tile, tid, g);
      __syncthreads();
      store_grad_tile<kBf16>(tile, a.grad, cell0, cells_here, tid);
    }
    __syncthreads();
  }
  block_sum_to_partials(local, a.partials);
}

// out = (total, mse, aiur, cl)
__global__ __launch_bounds__(256) void smr_loss_finish_kernel(const double* __restrict__ partials, int blocks,
                                                              const int* __restrict__ frame_counts,
                                                              const int* __restrict__ true_count, int frames,
                                                              const int* __restrict__ frames_with_events,
                                                              int cells_per_frame, double inv_elements, float w_class,
                                                              float w_aiur, float w_cl, float* __restrict__ out) {
  double iou = 0.0;
  for (int f = threadIdx.x; f < frames; f += 256) {
    const float inter = static_cast<float>(frame_counts[2 * f + 1]);
    const float uni = static_cast<float>(frame_counts[2 * f]) + static_cast<float>(true_count[f]) - inter;
    iou += uni > 0.0f ? static_cast<double>(inter / (uni + 1e-8f)) : 1.0;       // fp32 quotient like the reference
  }
  double s[3] = {strided_sum_256(partials, blocks), strided_sum_256(partials + blocks, blocks), iou};   // sq, cl, iou
  tree_sum_256(s);
  if (threadIdx.x == 0) {
    const float mse = static_cast<float>(s[0] * inv_elements);
    const float aiur = 1.0f - static_cast<float>(s[2] / frames);
    const float denom = static_cast<float>(*frames_with_events) * static_cast<float>(cells_per_frame) + 1e-10f;
    const float clv = static_cast<float>(s[1]) / denom;
    // w_class * mse + w_aiur * aiur + w_cl * clv with the multiply-adds spelled out: which product the compiler rounds
    // on its own otherwise changes with the code around it, and the total with it, by one ulp
    out[0] = fmaf(w_cl, clv, fmaf(w_class, mse, w_aiur * aiur));
    out[1] = mse;
    out[2] = aiur;
    out[3] = clv;
  }
}

}  // namespace

}  // namespace seld

extern "C" {

int64_t seld_smr_loss_workspace_bytes(int64_t frames, int64_t cells_per_frame) {
  if (frames <= 0 || cells_per_frame <= 0) return 0;
  // attention map (float per cell) | true counts (int per frame) | frame counts (2 ints per frame) | frames with events
  // (1 int, padded) | partial sums (2 x 4096 doubles)
  return frames * cells_per_frame * 4 + frames * 4 + frames * 8 + 16 + 2 * seld::kLossMaxPartials * 8 + 64;
}

int seld_smr_loss(const void* logits, int logits_is_bf16, const uint16_t* mask, const float* dense_labels,
                  int64_t frames, int rows, int cols, int num_classes, float w_class, float w_aiur, float w_cl,
                  float* loss_out4, void* grad, void* workspace, void* stream_) {
  using namespace seld;
  const int64_t cells = static_cast<int64_t>(rows) * cols;
  const bool bad_shape = frames <= 0 || rows < 3 || cols < 3 || cells > kL3MaxCells;
  const int64_t n_cells = bad_shape ? 0 : frames * cells;
  DeviceState* st;
  const int rc = check_class_loss_args(
      "seld_smr_loss", num_classes, bad_shape ? "frames > 0, a grid of at least 3 x 3 and at most 1024 cells" : nullptr,
      "cells * classes", n_cells, logits, loss_out4, workspace, mask, dense_labels, &st);
  if (rc != kOk) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  float* att = reinterpret_cast<float*>(ws);
  int* true_count = reinterpret_cast<int*>(ws + n_cells * 4);
  int* frame_counts = true_count + frames;
  int* n_event_frames = frame_counts + 2 * frames;
  size_t off = static_cast<size_t>(n_cells) * 4 + static_cast<size_t>(frames) * 12 + 16;
  off = (off + 63) / 64 * 64;
  double* partials = reinterpret_cast<double*>(ws + off);
  SELD_HIP_TRY(hipMemsetAsync(n_event_frames, 0, sizeof(int), stream));
  if (mask) hipLaunchKernelGGL(cl_prepare_kernel<true>, dim3(static_cast<unsigned>(frames)), dim3(kLossBlock), 0, stream,
                               mask, dense_labels, rows, cols, att, true_count, frame_counts, n_event_frames);
  else hipLaunchKernelGGL(cl_prepare_kernel<false>, dim3(static_cast<unsigned>(frames)), dim3(kLossBlock), 0, stream, mask,
                          dense_labels, rows, cols, att, true_count, frame_counts, n_event_frames);
  const unsigned blocks = class_loss_blocks(st, n_cells);
  Loss3Args a{logits, mask, dense_labels, att, n_event_frames, frame_counts, static_cast<int>(n_cells),
              static_cast<int>(cells), grad ? w_class * 2.0f / (static_cast<float>(n_cells) * kLossClasses) : 0.0f, w_cl,
              partials, grad};
  dispatch_bools([&](auto bf16, auto mask_labels, auto with_grad) {
    hipLaunchKernelGGL((smr_loss_kernel<bf16.value, mask_labels.value, with_grad.value>), dim3(blocks), dim3(kLossBlock), 0,
                       stream, a);
  }, logits_is_bf16 != 0, mask != nullptr, grad != nullptr);
  hipLaunchKernelGGL(smr_loss_finish_kernel, dim3(1), dim3(256), 0, stream, partials, static_cast<int>(blocks),
                     frame_counts, true_count, static_cast<int>(frames), n_event_frames, static_cast<int>(cells),
                     1.0 / (static_cast<double>(n_cells) * kLossClasses), w_class, w_aiur, w_cl, loss_out4);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
