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
//     channels of one position; the epilogue swaps halves between neighbouring 16-lane rows (v_permlane16_swap_b32) so
//     that a lane stores eight consecutive channels: 16-byte stores, half as many of them.
//   * the next stage's weight slice is requested (scalar base + one 32-bit offset per thread) behind the second barrier,
//     ahead of the stage's first MFMA, and waited for behind its last; the position fragments are read two (four with
//     the 64-wide tile) steps of kNTiles MFMAs ahead and the weight fragments of the second K half during the first, so
//     the LDS waits inside a stage are counted ones.  The compiler keeps neither by itself (it used to issue the loads
//     at the loop header and wait for them right behind the barrier, and to read each fragment just ahead of its
//     MFMAs): scheduling fences hold the order and tests/test_conv_loop_schedule_cpu.py reads it off the assembly.
//     Two workgroups per CU, one stages while the other multiplies.  The image is still loaded and stored in two
//     batches at the top of tap 0 (requesting the first batch under the previous tap's MFMAs was measured: no gain).
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

#include "conv3x3_image.h"
#include "seld_bf16.h"

namespace seld {
namespace conv3x3 {

constexpr int kLoopP = 256;          // positions per workgroup
constexpr int kLoopKc = kChannels;   // K channels per stage
constexpr int kLoopMaxChannels = 1 << 20;   // a weight piece's byte offset inside its slice (< 64 rows of 9 * C) is 32-bit

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
  static constexpr int kAhead = NT == 128 ? 2 : 4;              // steps a position fragment is read ahead (>= 8 MFMAs)
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

  // the prefetched weight slice lives across the loop's back edge: named registers (as an array it stays in scratch).
  // A piece's address is a wave-uniform base (the stage's tap and K slice, and the piece's row group: scalar registers)
  // plus one 32-bit byte offset per thread that is the same for every piece and stage: no address registers live
  // across the loop and no vector multiplies between the MFMAs.
  static_assert(G::kWLoads == 2 || G::kWLoads == 4, "weight pieces per thread");
  constexpr int kWPieceRows = kFwd ? kThreads / 8 : kThreads / (NT / 8);        // slice rows between a thread's pieces
  const long w_row = 9L * (kFwd ? Ck : Cn);                                     // elements per slice row
  const unsigned w_voff = kFwd ? ((tid >> 3) * 9 * Ck + (tid & 7) * 8) * 2u
                               : ((tid / (NT / 8)) * 9 * Cn + (tid % (NT / 8)) * 8) * 2u;
  u32x4 rw0, rw1, rw2 = u32x4{0u, 0u, 0u, 0u}, rw3 = rw2;
  auto w_piece = [&](const unsigned short* base, int i, unsigned voff) {
    return *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(base + i * kWPieceRows * w_row) + voff);
  };
  auto load_w = [&](int stage) {
    // the offset's widening must stay beside the loads for the scalar-base form of the load to be chosen: hoisted
    // out of the loop it comes back as four 64-bit vector addresses per stage
    unsigned voff = w_voff;
    asm volatile("" : "+v"(voff));
    const int kc = stage / 9, tap = stage - kc * 9;
    const unsigned short* const base = kFwd ? w + (n0 * 9L + tap) * Ck + kc * kLoopKc
                                            : w + (kc * kLoopKc * 9L + tap) * Cn + n0;
    rw0 = w_piece(base, 0, voff);
    rw1 = w_piece(base, 1, voff);
    if constexpr (G::kWLoads == 4) {
      rw2 = w_piece(base, 2, voff);
      rw3 = w_piece(base, 3, voff);
    }
  };
  auto w_slot = [&](int i) {
    const int piece = tid + i * kThreads;
    if constexpr (kFwd) return reinterpret_cast<u32x4*>(lw + (piece >> 3) * G::kWPitch + (piece & 7) * 8);
    else return reinterpret_cast<u32x4*>(lw + piece / (NT / 8) * G::kWPitch + piece % (NT / 8) * 8);
  };

  const int stages = Ck / kLoopKc * 9;
  load_w(0);
  for (int stage = 0; stage < stages; ++stage) {
    const int kc = stage / 9, tap = stage - kc * 9;
    // the image goes through registers in two batches (all of it beside the accumulators would spill); the first
    // is in flight while the other waves finish the previous stage
    uint4 rimg[G::kImgBatch];
    auto load_img = [&](int first) {
      // the pieces' addresses and bounds are derived again for every image (once per nine stages) behind an empty
      // asm: kept over the loop they would cost twelve registers beside the accumulators
      int t = tid;
      asm volatile("" : "+v"(t));
#pragma unroll
      for (int i = 0; i < G::kImgBatch; ++i)
        rimg[i] = image_piece<F, kLoopP>(src, clip_row, t0, T, Ck, kc * kLoopKc, t + (first + i) * kThreads);
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
    // the next slice is requested here, ahead of this stage's first MFMA, and waited for behind its last (the last
    // stage fetches its own slice again: no branch).  Nothing may move across the fence; without it and the use of
    // the registers below, the compiler merges these loads with the ones ahead of the loop and issues them at the
    // loop header, where every stage waits a full load latency for them behind the barrier.
    load_w(min(stage + 1, stages - 1));
    __builtin_amdgcn_sched_barrier(0);

    // forward reads src at (t + r - 1, f + s - 1); the data gradient at (t + 1 - r, f + 1 - s): the mirrored offset
    const int shift = (kFwd ? tap_shift<F>(tap) : -tap_shift<F>(tap)) * kPitch;
    // a stage is 16 steps (ks, m) of kNTiles MFMAs.  The position fragment of a step is read kAhead steps before
    // its MFMAs and the weight fragments of ks = 1 during the first steps of ks = 0, so the waits are counted
    // (lgkmcnt(N > 0)) instead of one full LDS latency per step.  A fence after every step keeps that order.
    constexpr int kSteps = 8 * (kLoopKc / 32);
    constexpr int kAhead = G::kAhead;
    auto read_w = [&](int ks, int n) {
      if constexpr (kFwd)
        return *reinterpret_cast<const bf16x8*>(lw + w_off + n * 16 * G::kWPitch + ks * 32);
      else
        return join(tr_read(lw, w_off + ks * 32 * G::kWPitch + n * 16),
                    tr_read(lw, w_off + (ks * 32 + 16) * G::kWPitch + n * 16));
    };
    auto read_d = [&](int step) {
      return *reinterpret_cast<const bf16x8*>(limg + d_off + d_rows(step & 7) * kPitch + shift + (step >> 3) * 32);
    };
    bf16x8 wf[kLoopKc / 32][G::kNTiles], df[kAhead + 1];
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n) wf[0][n] = read_w(0, n);
#pragma unroll
    for (int a = 0; a < kAhead; ++a) df[a] = read_d(a);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int step = 0; step < kSteps; ++step) {
      const int ks = step >> 3, m = step & 7;
      if (step + kAhead < kSteps) df[(step + kAhead) % (kAhead + 1)] = read_d(step + kAhead);
      if (ks + 1 < kLoopKc / 32 && m < G::kNTiles) wf[ks + 1][m] = read_w(ks + 1, m);
#pragma unroll
      for (int n = 0; n < G::kNTiles; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks][n], df[step % (kAhead + 1)], acc[m][n], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the prefetched slice is due here, not earlier
    asm volatile("" : "+v"(rw0), "+v"(rw1));
    if constexpr (G::kWLoads == 4) asm volatile("" : "+v"(rw2), "+v"(rw3));
  }

  // C/D of the 16x16 tile: column (position) = lane & 15, rows (result channel) = 4 * (lane >> 4) + j.  Two position
  // tiles are stored together: the 16-lane rows g and g + 1 (g even) hold channels 4g .. 4g+3 and 4g+4 .. 4g+7 of the
  // same positions, and v_permlane16_swap_b32 hands row g the other row's half of tile 2k and row g + 1 the other
  // row's half of tile 2k + 1, so every lane stores 8 consecutive channels of one position: half as many store
  // instructions of 16 bytes (the tail of 8-byte stores was issue-bound), the same bytes at the same addresses.
  const int rows_left = (T - t0) * F;                           // positions of the chunk inside the clip
  unsigned short* const out = dst + ((clip_row + t0) * F) * Cn + n0 + wn * (NT / 2) + 4 * (g & ~1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pos = wm * 128 + (2 * k + (g & 1)) * 16 + l15;
#pragma unroll
    for (int n = 0; n < G::kNTiles; ++n) {
      const f32x4 v0 = acc[2 * k][n], v1 = acc[2 * k + 1][n];
      // [0]: rows 0, 2 keep their value of tile 2k, rows 1, 3 receive rows 0, 2's value of tile 2k + 1;
      // [1]: rows 0, 2 receive rows 1, 3's value of tile 2k, rows 1, 3 keep their value of tile 2k + 1
      const u32x2 lo =
          __builtin_amdgcn_permlane16_swap(pack_bf16x2(v0[0], v0[1]), pack_bf16x2(v1[0], v1[1]), false, false);
      const u32x2 hi =
          __builtin_amdgcn_permlane16_swap(pack_bf16x2(v0[2], v0[3]), pack_bf16x2(v1[2], v1[3]), false, false);
      if (pos < rows_left)
        *reinterpret_cast<u32x4*>(out + static_cast<long>(pos) * Cn + n * 16) = u32x4{lo[0], hi[0], lo[1], hi[1]};
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
          const float v = round_bf16(acc[m][n][j]);
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
