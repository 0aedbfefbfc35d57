// Forward of the encoder's 3x3 / stride 1 / pad 1 / bias-free convolutions (model_crnn.py:5-17, ConvBlock.conv) on
// channels-last bf16 tensors, on the data-gradient kernel's main loop (conv3x3_loop.h), with the BatchNorm statistics
// of the following tail (convtail.hip) formed in the epilogue:
//
//   y[b][t][f][co] = sum over (r, s, ci) of x[b][t + r - 1][f + s - 1][ci] * W[co][r][s][ci]   (zero outside the map)
//
// an implicit GEMM with M = B * T * F positions, N = Cout and K = 9 * Cin.  The weights are read where they lie: the
// slice W[co0 .. co0+NT][r][s][ci0 .. ci0+64] of a stage has k contiguous like the image rows, so both operands are
// staged as plain 16-byte pieces and read with one ds_read_b128 per fragment (no weight transform launch).
//
// kStats: the convolution output is what tail_stats_kernel would read back from memory a moment later; the epilogue
// sums the values it stores (as rounded to bf16) and their squares per output channel over the chunk's valid positions
// and writes one partial row per chunk, which seld_conv_tail_forward_from_partials finalises in double.  The sums are
// unshifted, as in convfirst.hip: a chunk does not know the first row of the map, and one chunk's 256 exact squares of
// 8-bit significands summed pairwise in fp32 lose nothing the shifted pass would keep (DESIGN 5.5 has the measured
// errors of both).
#include <hip/hip_bf16.h>

#include "conv3x3_loop.h"
#include "seld_common.h"

namespace seld {

namespace {

using namespace conv3x3;

template <int F, int NT, bool kStats>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_fwd_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w, int T, int Cin, int Cout,
    int chunks_per_clip, unsigned short* __restrict__ y, float* __restrict__ partials) {
  conv3x3_loop<F, NT, true, kStats>(x, w, T, Cout, Cin, chunks_per_clip, y, partials);
}

bool fwd_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return (F == 8 || F == 16 || F == 32) && Cin > 0 && Cout > 0 && Cin % kLoopKc == 0 && Cout % 64 == 0 &&
         Cin <= kLoopMaxChannels && Cout <= kLoopMaxChannels;
}

int64_t fwd_chunks(int64_t B, int64_t T, int64_t F) {
  const int64_t tc = kLoopP / F;
  return B * ((T + tc - 1) / tc);
}

template <int F, int NT>
void launch_fwd_tile(const unsigned short* x, const unsigned short* w, int T, int Cin, int Cout, int chunks_per_clip,
                     unsigned chunks, unsigned short* y, float* partials, hipStream_t stream) {
  const dim3 grid(chunks, static_cast<unsigned>(Cout / NT));
  if (partials)
    hipLaunchKernelGGL((conv3x3_fwd_kernel<F, NT, true>), grid, dim3(kThreads), 0, stream, x, w, T, Cin, Cout,
                       chunks_per_clip, y, partials);
  else
    hipLaunchKernelGGL((conv3x3_fwd_kernel<F, NT, false>), grid, dim3(kThreads), 0, stream, x, w, T, Cin, Cout,
                       chunks_per_clip, y, partials);
}

template <int F>
void launch_fwd(const unsigned short* x, const unsigned short* w, int B, int T, int Cin, int Cout, unsigned short* y,
                float* partials, hipStream_t stream) {
  constexpr int tc = kLoopP / F;
  const int chunks_per_clip = (T + tc - 1) / tc;
  const unsigned chunks = static_cast<unsigned>(B * chunks_per_clip);
  if (Cout % 128 == 0) launch_fwd_tile<F, 128>(x, w, T, Cin, Cout, chunks_per_clip, chunks, y, partials, stream);
  else launch_fwd_tile<F, 64>(x, w, T, Cin, Cout, chunks_per_clip, chunks, y, partials, stream);
}

}  // namespace

}  // namespace seld

extern "C" {

int seld_conv3x3_forward_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return seld::fwd_supported(F, Cin, Cout) ? 1 : 0;
}

int64_t seld_conv3x3_forward_chunks(int64_t B, int64_t T, int64_t F) {
  if (!(F == 8 || F == 16 || F == 32) || B <= 0 || T <= 0) return 0;
  return seld::fwd_chunks(B, T, F);
}

int seld_conv3x3_forward(const void* x, const void* w, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                         void* y, float* partials, void* stream_) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!x || !w || !y || B <= 0 || T <= 0) return fail(kErrInvalidArgument, "seld_conv3x3_forward: bad argument");
  if (!fwd_supported(F, Cin, Cout))
    return fail(kErrUnsupported, "seld_conv3x3_forward: F in {8, 16, 32} and channel counts % 64 == 0 required");
  if (fwd_chunks(B, T, F) > 0x7fffffffLL || B * T > 0x7fffffffLL)
    return fail(kErrUnsupported, "seld_conv3x3_forward: too many positions");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15) != 0)
    return fail(kErrInvalidArgument, "seld_conv3x3_forward: 16-byte aligned tensors required");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned short* xs = static_cast<const unsigned short*>(x);
  const unsigned short* ws = static_cast<const unsigned short*>(w);
  unsigned short* ys = static_cast<unsigned short*>(y);
  const int b = static_cast<int>(B), t = static_cast<int>(T), ci = static_cast<int>(Cin), co = static_cast<int>(Cout);
  switch (F) {
    case 8: launch_fwd<8>(xs, ws, b, t, ci, co, ys, partials, stream); break;
    case 16: launch_fwd<16>(xs, ws, b, t, ci, co, ys, partials, stream); break;
    default: launch_fwd<32>(xs, ws, b, t, ci, co, ys, partials, stream); break;
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
