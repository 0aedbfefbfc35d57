// Data gradient of the encoder's 3x3 / stride 1 / pad 1 / bias-free convolutions (model_crnn.py:5-17, ConvBlock.conv)
// on channels-last bf16 tensors, from the weights where they lie (no flip / transpose launch):
//
//   dx[b][t][f][ci] = sum over (r, s, co) of dy[b][t + 1 - r][f + 1 - s][co] * W[co][r][s][ci]   (zero outside the map)
//
// an implicit GEMM with M = B * T * F positions, N = Cin and K = 9 * Cout.  The main loop is conv3x3_loop.h's (shared
// with the forward kernel of convfwd.hip), instantiated here in the data-gradient direction:
//
//   * a workgroup (4 waves, 2 x 2) owns kDgP = 256 positions (TC consecutive time rows of one clip) x NT input
//     channels (128, or 64 where Cin is not a multiple of 128) and walks K in stages of one tap x 64 output channels.
//   * the dy rows t0-1 .. t0+TC of a 64-channel slice are staged once per nine stages as the image of conv3x3_image.h
//     (the weight-gradient kernel's); the nine taps are nine row offsets into it, with the sign of the offset flipped.
//     The weights are not shared between taps: each stage stages its own [64 co][NT ci] slice W[co][r][s][ci0..], so
//     the output tile is GEMM-sized to keep the L2 -> LDS traffic per FLOP low.
//   * the weight slice has its rows over k (co) and ci contiguous: the fragments come from ds_read_b64_tr_b16 under
//     the k relabelling of conv3x3_image.h.  dy has k contiguous and takes one ds_read_b128 per fragment; to follow
//     the same relabelling the staging pass writes each 32-channel group of an image row in the order
//     0-3, 16-19, 4-7, 20-23, 8-11, 24-27, 12-15, 28-31 (two 8-byte stores per 16-byte piece).
//   * the products are formed transposed, D[ci][pos] = W^T dy^T, so that a lane ends with four consecutive input
//     channels of one position; neighbouring lane rows swap halves and a lane stores eight of them, 16 bytes.
//   * the next stage's weight slice is requested ahead of the current stage's MFMAs and waited for behind them
//     (conv3x3_loop.h says how that is held against the compiler); two workgroups per CU (at most 72 832 B of LDS
//     each), one stages while the other multiplies.
//   * v_mfma_f32_16x16x32_bf16, fp32 accumulation over all of K in a fixed order, one rounding, every output written
//     once: no atomics, no split-K, the same inputs give the same bits.
#include <hip/hip_bf16.h>

#include "conv3x3_loop.h"
#include "seld_common.h"

namespace seld {

namespace {

using namespace conv3x3;

constexpr int kDgP = kLoopP;         // positions per workgroup
constexpr int kDgKc = kLoopKc;       // output channels per stage

// the shared loop in the data-gradient direction (mirrored tap offset, transposed weight reads), plain store
template <int F, int NT>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_dgrad_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ w, int T, int Cin, int Cout,
    int chunks_per_clip, unsigned short* __restrict__ dx) {
  conv3x3_loop<F, NT, false, false>(dy, w, T, Cin, Cout, chunks_per_clip, dx, nullptr);
}

bool dgrad_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return (F == 8 || F == 16 || F == 32) && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % kDgKc == 0 &&
         Cin <= kLoopMaxChannels && Cout <= kLoopMaxChannels;
}

template <int F>
void launch_dgrad(const unsigned short* dy, const unsigned short* w, int B, int T, int Cin, int Cout,
                  unsigned short* dx, hipStream_t stream) {
  constexpr int tc = kDgP / F;
  const int chunks_per_clip = (T + tc - 1) / tc;
  const unsigned chunks = static_cast<unsigned>(B * chunks_per_clip);
  if (Cin % 128 == 0)
    hipLaunchKernelGGL((conv3x3_dgrad_kernel<F, 128>), dim3(chunks, static_cast<unsigned>(Cin / 128)), dim3(kThreads),
                       0, stream, dy, w, T, Cin, Cout, chunks_per_clip, dx);
  else
    hipLaunchKernelGGL((conv3x3_dgrad_kernel<F, 64>), dim3(chunks, static_cast<unsigned>(Cin / 64)), dim3(kThreads), 0,
                       stream, dy, w, T, Cin, Cout, chunks_per_clip, dx);
}

}  // namespace

}  // namespace seld

extern "C" {

int seld_conv3x3_dgrad_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return seld::dgrad_supported(F, Cin, Cout) ? 1 : 0;
}

int seld_conv3x3_dgrad(const void* dy, const void* w, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                       void* dx, void* stream_) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!dy || !w || !dx || B <= 0 || T <= 0) return fail(kErrInvalidArgument, "seld_conv3x3_dgrad: bad argument");
  if (!dgrad_supported(F, Cin, Cout))
    return fail(kErrUnsupported, "seld_conv3x3_dgrad: F in {8, 16, 32} and channel counts % 64 == 0 required");
  if (B * ((T + kDgP / F - 1) / (kDgP / F)) > 0x7fffffffLL || B * T > 0x7fffffffLL)
    return fail(kErrUnsupported, "seld_conv3x3_dgrad: too many positions");
  if (((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(dx)) & 15) != 0)
    return fail(kErrInvalidArgument, "seld_conv3x3_dgrad: 16-byte aligned tensors required");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned short* ds = static_cast<const unsigned short*>(dy);
  const unsigned short* ws = static_cast<const unsigned short*>(w);
  unsigned short* xs = static_cast<unsigned short*>(dx);
  const int b = static_cast<int>(B), t = static_cast<int>(T), ci = static_cast<int>(Cin), co = static_cast<int>(Cout);
  switch (F) {
    case 8: launch_dgrad<8>(ds, ws, b, t, ci, co, xs, stream); break;
    case 16: launch_dgrad<16>(ds, ws, b, t, ci, co, xs, stream); break;
    default: launch_dgrad<32>(ds, ws, b, t, ci, co, xs, stream); break;
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
