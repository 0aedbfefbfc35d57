// Data gradient of the encoder's 3x3 / stride 1 / pad 1 / bias-free convolutions (model_crnn.py:5-17, ConvBlock.conv)
// on channels-last bf16 tensors, from the weights where they lie (no flip / transpose launch):
//
//   dx[b][t][f][ci] = sum over (r, s, co) of dy[b][t + 1 - r][f + 1 - s][co] * W[co][r][s][ci]   (zero outside the map)
//
// an implicit GEMM with M = B * T * F positions, N = Cin and K = 9 * Cout.
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
//     channels of one position: 8-byte stores, no shuffle.
//   * the next stage's weight slice is fetched into registers while the current one multiplies; two workgroups per CU
//     (at most 72 832 B of LDS each), one stages while the other multiplies.
//   * v_mfma_f32_16x16x32_bf16, fp32 accumulation over all of K in a fixed order, one rounding, every output written
//     once: no atomics, no split-K, the same inputs give the same bits.
#include <hip/hip_bf16.h>

#include "conv3x3_image.h"
#include "seld_common.h"

namespace seld {

namespace {

using namespace conv3x3;

constexpr int kDgP = 256;            // positions per workgroup
constexpr int kDgKc = kChannels;     // output channels per stage

template <int F, int NT>
struct DgradGeom {
  static_assert(NT == 64 || NT == 128, "input channels per workgroup: 64 or 128");
  using Img = Image<F, kDgP>;
  static constexpr int kWPitch = NT + 16;                    // weight rows: 288 B / 160 B, 8 rows cover the banks
  static constexpr int kWLoads = kDgKc * NT / 8 / kThreads;  // 16-byte pieces per thread and stage
  static constexpr int kNTiles = NT / 32;                    // 16-channel tiles per wave
  static constexpr int kImgBatch = (Img::kLoads + 1) / 2;     // 16-byte image pieces per thread and batch
  static constexpr int kImgShorts = Img::kRows * kPitch;
  static constexpr int kLdsShorts = kImgShorts + kDgKc * kWPitch;
  static_assert(2 * kLdsShorts * 2 <= 160 * 1024, "two workgroups per CU");
};

template <int F, int NT>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_dgrad_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ w, int T, int Cin, int Cout,
    int chunks_per_clip, unsigned short* __restrict__ dx) {
  using G = DgradGeom<F, NT>;
  __shared__ __attribute__((aligned(16))) unsigned short lds[G::kLdsShorts];
  unsigned short* const limg = lds;
  unsigned short* const lw = lds + G::kImgShorts;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int chunk = blockIdx.x, ci0 = blockIdx.y * NT;
  const int b = chunk / chunks_per_clip, t0 = (chunk - b * chunks_per_clip) * G::Img::TC;
  const long clip_row = static_cast<long>(b) * T;

  f32x4 acc[8][G::kNTiles];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n) acc[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, l15 = lane & 15;
  const int w_off = (4 * g + q) * G::kWPitch + wn * (NT / 2) + 4 * p;       // transposed weight reads (first half)
  // dy fragment of position tile m: 16 positions further = a constant number of image rows for every F
  const int d_off = image_row<F>(wm * 128 + l15) * kPitch + 8 * g;
  auto d_rows = [](int m) { return image_row<F>(16 * m) - image_row<F>(0); };

  // the prefetched weight slice lives across the loop's back edge: named registers (as an array it stays in scratch)
  static_assert(G::kWLoads == 2 || G::kWLoads == 4, "weight pieces per thread");
  uint4 rw0, rw1, rw2 = make_uint4(0u, 0u, 0u, 0u), rw3 = rw2;
  auto w_piece = [&](int stage, int i) {
    const int kc = stage / 9, tap = stage - kc * 9;
    const int piece = tid + i * kThreads, row = piece / (NT / 8), ch = piece % (NT / 8);
    return *reinterpret_cast<const uint4*>(w + (static_cast<long>(kc * kDgKc + row) * 9 + tap) * Cin + ci0 + ch * 8);
  };
  auto load_w = [&](int stage) {
    rw0 = w_piece(stage, 0);
    rw1 = w_piece(stage, 1);
    if constexpr (G::kWLoads == 4) {
      rw2 = w_piece(stage, 2);
      rw3 = w_piece(stage, 3);
    }
  };
  auto w_slot = [&](int i) {
    const int piece = tid + i * kThreads;
    return reinterpret_cast<uint4*>(lw + piece / (NT / 8) * G::kWPitch + piece % (NT / 8) * 8);
  };

  const int stages = Cout / kDgKc * 9;
  load_w(0);
  for (int stage = 0; stage < stages; ++stage) {
    const int kc = stage / 9, tap = stage - kc * 9;
    // the image goes through registers in two batches (all of it beside the accumulators would spill); the first
    // is in flight while the other waves finish the previous stage
    uint4 rimg[G::kImgBatch];
    auto load_img = [&](int first) {
#pragma unroll
      for (int i = 0; i < G::kImgBatch; ++i)
        rimg[i] = image_piece<F, kDgP>(dy, clip_row, t0, T, Cout, kc * kDgKc, tid + (first + i) * kThreads);
    };
    auto store_img = [&](int first) {
#pragma unroll
      for (int i = 0; i < G::kImgBatch; ++i) {
        const int piece = tid + (first + i) * kThreads, ch = piece & 7;
        // channels 8h .. 8h+3 and 8h+4 .. 8h+7 of a 32-channel group go to its slots 16(h&1) + 4(h>>1) and 8 further
        unsigned short* const dst = limg + (piece >> 3) * kPitch + (ch >> 2) * 32 + 16 * (ch & 1) + 4 * ((ch >> 1) & 1);
        if (piece < G::Img::kRows * 8) {
          *reinterpret_cast<uint2*>(dst) = make_uint2(rimg[i].x, rimg[i].y);
          *reinterpret_cast<uint2*>(dst + 8) = make_uint2(rimg[i].z, rimg[i].w);
        }
      }
    };
    if (tap == 0) load_img(0);
    __syncthreads();                                            // the previous stage's fragment reads are done
    *w_slot(0) = rw0;
    *w_slot(1) = rw1;
    if constexpr (G::kWLoads == 4) {
      *w_slot(2) = rw2;
      *w_slot(3) = rw3;
    }
    if (tap == 0) {
      store_img(0);
      load_img(G::kImgBatch);
      store_img(G::kImgBatch);
    }
    __syncthreads();
    load_w(min(stage + 1, stages - 1));                         // in flight under this stage's products (the last
                                                                // stage fetches its own slice again: no branch)

    // dy is read at (t + 1 - r, f + 1 - s): the mirrored offset of tap (r, s)
    const int shift = -tap_shift<F>(tap) * kPitch;
#pragma unroll
    for (int ks = 0; ks < kDgKc / 32; ++ks) {
      bf16x8 wf[G::kNTiles];
#pragma unroll
      for (int n = 0; n < G::kNTiles; ++n)
        wf[n] = join(tr_read(lw, w_off + ks * 32 * G::kWPitch + n * 16),
                     tr_read(lw, w_off + (ks * 32 + 16) * G::kWPitch + n * 16));
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const bf16x8 df = *reinterpret_cast<const bf16x8*>(limg + d_off + d_rows(m) * kPitch + shift + ks * 32);
#pragma unroll
        for (int n = 0; n < G::kNTiles; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], df, acc[m][n], 0, 0, 0);
      }
    }
  }

  // C/D of the 16x16 tile: column (position) = lane & 15, rows (ci) = 4 * (lane >> 4) + j
  const int rows_left = (T - t0) * F;                           // positions of the chunk inside the clip
  unsigned short* const out = dx + ((clip_row + t0) * F) * Cin + ci0 + wn * (NT / 2) + 4 * g;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int pos = wm * 128 + m * 16 + l15;
    if (pos >= rows_left) continue;
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n) {
      const f32x4 v = acc[m][n];
      const unsigned lo = static_cast<unsigned>(__bfloat16_as_ushort(__float2bfloat16(v[0]))) |
                          (static_cast<unsigned>(__bfloat16_as_ushort(__float2bfloat16(v[1]))) << 16);
      const unsigned hi = static_cast<unsigned>(__bfloat16_as_ushort(__float2bfloat16(v[2]))) |
                          (static_cast<unsigned>(__bfloat16_as_ushort(__float2bfloat16(v[3]))) << 16);
      *reinterpret_cast<uint2*>(out + static_cast<long>(pos) * Cin + n * 16) = make_uint2(lo, hi);
    }
  }
}

bool dgrad_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return (F == 8 || F == 16 || F == 32) && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % kDgKc == 0;
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
