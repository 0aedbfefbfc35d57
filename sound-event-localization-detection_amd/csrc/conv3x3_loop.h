// The implicit-GEMM main loop shared by the data-gradient kernel (convdgrad.hip) and the forward kernel (convfwd.hip)
// of the encoder's 3x3 / stride 1 / pad 1 / bias-free convolutions on channels-last bf16 tensors.
//
//   * a workgroup (4 waves, 2 x 2) owns kLoopP = 256 positions (TC consecutive time rows of one clip) x NT channels of
//     the result (128, or 64 where their count is not a multiple of 128) and walks K in stages of one tap x 64 channels
//     of the staged activation `src` (Ck channels; the result has Cn).
//   * the src rows t0-1 .. t0+TC of a 64-channel slice are staged once per nine stages as the image of conv3x3_image.h;
//     the nine taps are nine row offsets into it.  The weights are not shared between taps: each stage stages its own
//     slice, so the output tile is GEMM-sized to keep the L2 -> LDS traffic per FLOP low.
//   * the products are formed transposed, D[n][pos] = W-slice x src^T, so that a lane ends with four consecutive result
//     channels of one position: 8-byte stores, no shuffle.
//   * the next stage's weight slice is fetched into registers while the current one multiplies; two workgroups per CU,
//     one stages while the other multiplies.
//   * v_mfma_f32_16x16x32_bf16, fp32 accumulation over all of K in a fixed order, one rounding, every output written
//     once: no atomics, no split-K, the same inputs give the same bits.
//
// kFwd = false (data gradient: src = dy, Ck = Cout, Cn = Cin):
//     dx[b][t][f][ci] = sum over (r, s, co) of dy[b][t + 1 - r][f + 1 - s][co] * W[co][r][s][ci]
//   the tap offset is mirrored; the slice W[co0 .. co0+64][r][s][ci0 .. ci0+NT] has its rows over k and the result channel
//   contiguous: the fragments come from ds_read_b64_tr_b16 under the k relabelling of conv3x3_image.h, and to follow the
//   same relabelling the staging pass writes each 32-channel group of an image row in the order 0-3, 16-19, 4-7, 20-23,
//   8-11, 24-27, 12-15, 28-31 (two 8-byte stores per 16-byte piece).
// kFwd = true (forward: src = x, Ck = Cin, Cn = Cout):
//     y[b][t][f][co] = sum over (r, s, ci) of x[b][t + r - 1][f + s - 1][ci] * W[co][r][s][ci]
//   the slice W[co0 .. co0+NT][r][s][ci0 .. ci0+64] has its rows over the result channel and k contiguous, like the image
//   rows: both are staged as plain 16-byte pieces at the 160-byte pitch and read with one ds_read_b128 per fragment (the
//   relabelling is the identity on both operands).  No weight transform of any kind.
// kStats (forward only): the epilogue also forms, from the values as rounded to bf16 for the store, the sum and the sum
// of squares per result channel over the valid positions of the chunk (the lane's 8 position tiles pairwise, the 16
// lanes of a row by a butterfly, the two waves that share the channels through LDS: a fixed order, no atomics) and
// writes them as row `chunk` of partials[stat][chunks][Cn].
#pragma once

#include <hip/hip_bf16.h>

#include "conv3x3_image.h"

namespace seld {
namespace conv3x3 {

constexpr int kLoopP = 256;          // positions per workgroup
constexpr int kLoopKc = kChannels;   // K channels per stage

template <int F, int NT, bool kFwd>
struct LoopGeom {
  static_assert(NT == 64 || NT == 128, "result channels per workgroup: 64 or 128");
  using Img = Image<F, kLoopP>;
  // weight rows: over k with 288 B / 160 B pitch (8 rows cover the banks), or over the result channel at the image's pitch
  static constexpr int kWPitch = kFwd ? kPitch : NT + 16;
  static constexpr int kWRows = kFwd ? NT : kLoopKc;
  static constexpr int kWLoads = kLoopKc * NT / 8 / kThreads;   // 16-byte pieces per thread and stage
  static constexpr int kNTiles = NT / 32;                       // 16-channel tiles per wave
  static constexpr int kImgBatch = (Img::kLoads + 1) / 2;       // 16-byte image pieces per thread and batch
  static constexpr int kImgShorts = Img::kRows * kPitch;
  static constexpr int kLdsShorts = kImgShorts + kWRows * kWPitch;
  static_assert(2 * kLdsShorts * 2 <= 160 * 1024, "two workgroups per CU");
};

// sum over the 16 lanes of a DPP row, every lane ends with the same bits (each step adds the same two values in
// either order)
template <int kCtrl>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kCtrl, 0xf, 0xf, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v = dpp_add<0xB1>(v);              // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);              // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);             // row_half_mirror: the other quad of the 8 lanes
  return dpp_add<0x140>(v);          // row_mirror: the other 8 lanes
}

template <int F, int NT, bool kFwd, bool kStats>
__device__ __forceinline__ void conv3x3_loop(const unsigned short* __restrict__ src, const unsigned short* __restrict__ w,
                                             int T, int Cn, int Ck, int chunks_per_clip,
                                             unsigned short* __restrict__ dst, float* __restrict__ partials) {
  static_assert(kFwd || !kStats, "the statistics epilogue belongs to the forward direction");
  using G = LoopGeom<F, NT, kFwd>;
  __shared__ __attribute__((aligned(16))) unsigned short lds[G::kLdsShorts];
  unsigned short* const limg = lds;
  unsigned short* const lw = lds + G::kImgShorts;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int chunk = blockIdx.x, n0 = blockIdx.y * NT;
  const int b = chunk / chunks_per_clip, t0 = (chunk - b * chunks_per_clip) * G::Img::TC;
  const long clip_row = static_cast<long>(b) * T;

  f32x4 acc[8][G::kNTiles];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n) acc[m][n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, l15 = lane & 15;
  const int w_off = kFwd ? (wn * (NT / 2) + l15) * G::kWPitch + 8 * g                 // row = result channel, 8 k
                         : (4 * g + q) * G::kWPitch + wn * (NT / 2) + 4 * p;          // transposed reads (first half)
  // src fragment of position tile m: 16 positions further = a constant number of image rows for every F
  const int d_off = image_row<F>(wm * 128 + l15) * kPitch + 8 * g;
  auto d_rows = [](int m) { return image_row<F>(16 * m) - image_row<F>(0); };

  // the prefetched weight slice lives across the loop's back edge: named registers (as an array it stays in scratch)
  static_assert(G::kWLoads == 2 || G::kWLoads == 4, "weight pieces per thread");
  uint4 rw0, rw1, rw2 = make_uint4(0u, 0u, 0u, 0u), rw3 = rw2;
  auto w_piece = [&](int stage, int i) {
    const int kc = stage / 9, tap = stage - kc * 9;
    const int piece = tid + i * kThreads;
    if constexpr (kFwd) {
      const int row = piece >> 3, ch = piece & 7;
      return *reinterpret_cast<const uint4*>(w + (static_cast<long>(n0 + row) * 9 + tap) * Ck + kc * kLoopKc + ch * 8);
    } else {
      const int row = piece / (NT / 8), ch = piece % (NT / 8);
      return *reinterpret_cast<const uint4*>(w + (static_cast<long>(kc * kLoopKc + row) * 9 + tap) * Cn + n0 + ch * 8);
    }
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
    if constexpr (kFwd) return reinterpret_cast<uint4*>(lw + (piece >> 3) * G::kWPitch + (piece & 7) * 8);
    else return reinterpret_cast<uint4*>(lw + piece / (NT / 8) * G::kWPitch + piece % (NT / 8) * 8);
  };

  const int stages = Ck / kLoopKc * 9;
  load_w(0);
  for (int stage = 0; stage < stages; ++stage) {
    const int kc = stage / 9, tap = stage - kc * 9;
    // the image goes through registers in two batches (all of it beside the accumulators would spill); the first
    // is in flight while the other waves finish the previous stage
    uint4 rimg[G::kImgBatch];
    auto load_img = [&](int first) {
#pragma unroll
      for (int i = 0; i < G::kImgBatch; ++i)
        rimg[i] = image_piece<F, kLoopP>(src, clip_row, t0, T, Ck, kc * kLoopKc, tid + (first + i) * kThreads);
    };
    auto store_img = [&](int first) {
#pragma unroll
      for (int i = 0; i < G::kImgBatch; ++i) {
        const int piece = tid + (first + i) * kThreads, ch = piece & 7;
        if constexpr (kFwd) {
          if (piece < G::Img::kRows * 8) *reinterpret_cast<uint4*>(limg + (piece >> 3) * kPitch + ch * 8) = rimg[i];
        } else {
          // channels 8h .. 8h+3 and 8h+4 .. 8h+7 of a 32-channel group go to its slots 16(h&1) + 4(h>>1) and 8 further
          unsigned short* const slot = limg + (piece >> 3) * kPitch + (ch >> 2) * 32 + 16 * (ch & 1) + 4 * ((ch >> 1) & 1);
          if (piece < G::Img::kRows * 8) {
            *reinterpret_cast<uint2*>(slot) = make_uint2(rimg[i].x, rimg[i].y);
            *reinterpret_cast<uint2*>(slot + 8) = make_uint2(rimg[i].z, rimg[i].w);
          }
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

    // forward reads src at (t + r - 1, f + s - 1); the data gradient at (t + 1 - r, f + 1 - s): the mirrored offset
    const int shift = (kFwd ? tap_shift<F>(tap) : -tap_shift<F>(tap)) * kPitch;
#pragma unroll
    for (int ks = 0; ks < kLoopKc / 32; ++ks) {
      bf16x8 wf[G::kNTiles];
#pragma unroll
      for (int n = 0; n < G::kNTiles; ++n) {
        if constexpr (kFwd)
          wf[n] = *reinterpret_cast<const bf16x8*>(lw + w_off + n * 16 * G::kWPitch + ks * 32);
        else
          wf[n] = join(tr_read(lw, w_off + ks * 32 * G::kWPitch + n * 16),
                       tr_read(lw, w_off + (ks * 32 + 16) * G::kWPitch + n * 16));
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const bf16x8 df = *reinterpret_cast<const bf16x8*>(limg + d_off + d_rows(m) * kPitch + shift + ks * 32);
#pragma unroll
        for (int n = 0; n < G::kNTiles; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n], df, acc[m][n], 0, 0, 0);
      }
    }
  }

  // C/D of the 16x16 tile: column (position) = lane & 15, rows (result channel) = 4 * (lane >> 4) + j
  const int rows_left = (T - t0) * F;                           // positions of the chunk inside the clip
  unsigned short* const out = dst + ((clip_row + t0) * F) * Cn + n0 + wn * (NT / 2) + 4 * g;
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
      *reinterpret_cast<uint2*>(out + static_cast<long>(pos) * Cn + n * 16) = make_uint2(lo, hi);
    }
  }

  if constexpr (kStats) {
    // the stored values again (same rounding), zero for the positions of a ragged chunk that lie outside the clip
    float* const red = reinterpret_cast<float*>(lds);           // [wm][stat][NT]
    __syncthreads();                                            // the last stage's fragment reads are done
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float r[8], s[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const float v = __uint_as_float(static_cast<unsigned>(__bfloat16_as_ushort(__float2bfloat16(acc[m][n][j]))) << 16);
          r[m] = wm * 128 + m * 16 + l15 < rows_left ? v : 0.0f;
          s[m] = r[m] * r[m];                                   // exact: 8-bit significands
        }
        const float s1 = row16_sum(((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])));
        const float s2 = row16_sum(((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])));
        if (l15 == 0) {
          const int c = wn * (NT / 2) + n * 16 + 4 * g + j;
          red[(wm * 2 + 0) * NT + c] = s1;
          red[(wm * 2 + 1) * NT + c] = s2;
        }
      }
    __syncthreads();
    if (tid < 2 * NT) {
      const int stat = tid / NT, c = tid - stat * NT;
      partials[(static_cast<long>(stat) * gridDim.x + chunk) * Cn + n0 + c] = red[stat * NT + c] + red[(2 + stat) * NT + c];
    }
  }
}

}  // namespace conv3x3
}  // namespace seld
