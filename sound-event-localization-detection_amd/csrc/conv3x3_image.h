// Shared pieces of the encoder's 3x3 / stride 1 / pad 1 convolution kernels on channels-last bf16 activations
// (convwgrad.hip, convdgrad.hip, convfwd.hip): a chunk of P positions = TC consecutive time rows of one clip is staged in LDS as an
// image [TC + 2][F + 2][64 channels] with zero rows outside [0, T) and a zero column on each frequency edge, so the
// nine taps are nine constant row offsets into it and nothing crosses a clip boundary.  Rows have a 160-byte pitch:
// eight consecutive rows then cover all 64 banks, which keeps the 32-lane halves of ds_read_b64_tr_b16 conflict-free
// under the k relabelling below.
#pragma once

#include <hip/hip_runtime.h>

namespace seld {
namespace conv3x3 {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kThreads = 256;
constexpr int kChannels = 64;        // channels per image row
constexpr int kPitch = 80;           // LDS row pitch in bf16: 64 channels + 16 pad = 160 B

template <int F, int P>
struct Image {
  static_assert(F == 8 || F == 16 || F == 32, "frequency bins: 8, 16 or 32");
  static_assert(P % F == 0, "a chunk is whole time rows");
  static constexpr int TC = P / F;                          // time rows per chunk
  static constexpr int kRows = (TC + 2) * (F + 2);          // image rows (with halo rows and edge columns)
  static constexpr int kLoads = (kRows * 8 + kThreads - 1) / kThreads;   // 16-byte pieces per thread
};

// image row of position `pos` of the chunk (the centre tap, i.e. no shift)
template <int F>
__device__ __forceinline__ int image_row(int pos) {
  return (pos / F + 1) * (F + 2) + pos % F + 1;
}

// row offset of tap (r, s) for a kernel that reads the input at (t + r - 1, f + s - 1)
template <int F>
__device__ __forceinline__ constexpr int tap_shift(int tap) {
  return (tap / 3 - 1) * (F + 2) + (tap % 3 - 1);
}

// 16-byte piece `piece` (image row piece / 8, channels c0 + 8 * (piece % 8) ..) of the image of the chunk that starts
// at time row t0 of the clip whose first row is clip_row; zero outside the map and past the image
template <int F, int P>
__device__ __forceinline__ uint4 image_piece(const unsigned short* __restrict__ src, long clip_row, int t0, int T,
                                             int C, int c0, int piece) {
  const int r = piece >> 3, ch = piece & 7;
  const int tr = r / (F + 2), f = r - tr * (F + 2) - 1, t = t0 - 1 + tr;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (r < Image<F, P>::kRows && t >= 0 && t < T && f >= 0 && f < F)
    v = *reinterpret_cast<const uint4*>(src + ((clip_row + t) * F + f) * C + c0 + ch * 8);
  return v;
}

// ds_read_b64_tr_b16: lane 4q+p of the 16-lane group g supplies row q, columns 4p..4p+3 of its 4-row block and
// receives column (lane & 15) of the four rows.  A K-group of 32 rows is read as two 4-row halves; the MFMA's k
// numbering is a free relabelling as long as both operands use the same one, so group g takes rows 4g..4g+3 and
// 16+4g..16+4g+3: a 32-lane half then reads 8 consecutive LDS rows.
__device__ __forceinline__ s16x4 tr_read(const unsigned short* base, int offset_shorts) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + offset_shorts));
}

__device__ __forceinline__ bf16x8 join(s16x4 lo, s16x4 hi) {
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace conv3x3
}  // namespace seld
