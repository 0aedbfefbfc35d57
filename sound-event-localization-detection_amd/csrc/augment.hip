// Training augmentation inside the device window gather for gfx950 -- pure data movement, bit-exact.
//
// The plain gather (labels.hip, gather_rows_kernel) copies 250-frame windows from the device timeline into the static
// input buffers of a captured step.  The kernels here do the same copy and, on the way, apply per window
//   * one of the 16 sign-and-swap transforms of the first-order-Ambisonics channels: an exact signed
//     permutation of the feature channels and an exact permutation of the DOA grid cells, and
//   * up to two time masks and two frequency masks (SpecAugment) on the features.
// The transform of window b is row b of a parameter table in device memory (SELD_AUGMENT_PARAM_INTS int32 per row):
//   [0] pattern p (0..15; 0 = identity): mirror m = p >> 3, then k = (p >> 1) & 3 quarter turns, then elevation flip e = p & 1
//   [1] [2] time mask 0: first frame, length      [3] [4] time mask 1
//   [5] [6] frequency mask 0: first bin, length   [7] [8] frequency mask 1
//   [9] azimuth step r: read by the rotating entry points only (permute_mask_kernel<true> below; rotate.hip for the features)
//   [10] [11] padding (ignored)
// A row is trusted no further than its bits: the pattern is reduced modulo 16 and the masks are only ever COMPARED with
// the coordinates the kernel itself generates, so no parameter value can move a load or a store.
//
// All kernels: one 16-byte store per thread and iteration, no LDS, no scratch, no atomics; blockIdx.y walks the windows,
// so a window's parameter row and start frame are wave-uniform (scalar loads).  The output of a window depends on
// (source, starts[b], params[b]) only.
#include "augment_core.h"

namespace seld {

// dst[b][w][c][f] = sign * src[starts[b] + w][srcch[c]][f], then the masks; rows past the timeline stay zero.
// kAffine (seld_window_gather_augment_affine): the copied value goes through scale / shift [channels][64] of the OUTPUT
// channel c before the masks (augment_core.h, standardised); the other instantiation never looks at the two pointers.
template <bool kAffine>
__global__ void __launch_bounds__(256)
gather_augment_kernel(const uint4* __restrict__ src, long total_rows, int channels, int freq_channels,
                      const int64_t* __restrict__ starts, const int32_t* __restrict__ params, long B, int window,
                      const ChannelTable table, unsigned mask_bits, const uint4* __restrict__ scale,
                      const uint4* __restrict__ shift, uint4* __restrict__ dst) {
  const int row_chunks = channels * kChunksPerChannel;
  const int per_window = window * row_chunks;                       // host: < 2^31
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    // up to 8 channels (every feature set with a defined swap): the pattern's table row is one wave-uniform 8-byte scalar
    // load and a lane picks its byte with a shift, so no per-lane table load sits in front of the data load
    const unsigned long long packed = *reinterpret_cast<const unsigned long long*>(table.e[prm.pattern]);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_chunks;
      const int chunk = q - w * row_chunks;
      const int c = chunk / kChunksPerChannel;
      const int fc = chunk - c * kChunksPerChannel;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        const unsigned entry = channels <= 8 ? packed_entry(packed, c) : table.e[prm.pattern][c];
        v = standardised<kAffine>(signed_copy(src + srow * row_chunks, entry, fc), scale, shift, chunk);
        v = masked(v, w, c, fc, prm, freq_channels, mask_bits);
      }
      to[q] = v;
    }
  }
}

// dst[b][w][cell'] = src[starts[b] + w][cell], cell -> cell' the window's grid permutation: a set cell (i, j) moves to
//   i' = e ? I-1-i : i,   j' = ((m ? J-1-j : j) + s) mod J,
// s = k J/4 cells, the pattern's quarter turns (seld_window_permute_mask: slot [9] of the row is not read), or with kStep
// s = (k J/4 + r) mod J, r the azimuth step of slot [9] (seld_window_permute_mask_rotate).
// Each thread builds 8 consecutive destination cells (one 16-byte store) from their source cells.  The identity (and any
// transform on a row past the timeline) keeps the 16-byte load of the plain gather; every other one reads 2-byte cells:
// J = 36 is not a multiple of 8, so a mirrored or rotated grid row has no 16-byte-aligned image in the source row.
template <bool kStep>
__global__ void __launch_bounds__(256)
permute_mask_kernel(const uint16_t* __restrict__ src, long total_rows, int I, int J, const int64_t* __restrict__ starts,
                    const int32_t* __restrict__ params, long B, int window, uint4* __restrict__ dst) {
  const int cells = I * J;
  const int row_chunks = cells / 8;
  const int per_window = window * row_chunks;                       // host: < 2^31
  const int quarter = J / 4;
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const int p = params[b * kParamInts] & (kPatterns - 1);
    const bool mirror = (p >> 3) != 0, flip = (p & 1) != 0;
    int shift = ((p >> 1) & 3) * quarter;
    if (kStep) shift = (shift + azimuth_step(params, b, J)) % J;
    const bool identity = kStep ? !mirror && !flip && shift == 0 : p == 0;
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_chunks;
      const int chunk = q - w * row_chunks;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        const uint16_t* __restrict__ row = src + srow * cells;
        if (identity) {
          v = reinterpret_cast<const uint4*>(row)[chunk];
        } else {
          int i2 = (chunk * 8) / J;                                 // destination cell (i2, j2)
          int j2 = chunk * 8 - i2 * J;
          unsigned h[8];
#pragma unroll
          for (int n = 0; n < 8; ++n) {
            const int i = flip ? I - 1 - i2 : i2;
            int jm = j2 - shift;
            jm = jm < 0 ? jm + J : jm;
            const int j = mirror ? J - 1 - jm : jm;
            h[n] = row[i * J + j];
            if (++j2 == J) { j2 = 0; ++i2; }
          }
          v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        }
      }
      to[q] = v;
    }
  }
}

// the two feature entry points
template <bool kAffine>
static int gather_augment(const char* who, const float* src, int64_t total_rows, int channels, int freq_channels,
                          const int64_t* starts, const int32_t* params, int64_t B, int64_t window,
                          const uint8_t* channel_table, float mask_value, const float* scale, const float* shift, float* dst,
                          void* stream_) {
  DeviceState* st;
  const int64_t row_chunks = static_cast<int64_t>(channels) * kChunksPerChannel;
  const bool extents_ok = channels > 0 && freq_channels >= 0 && freq_channels <= channels;
  const Refusal many{channels > kMaxChannels, kErrUnsupported, "more than SELD_AUGMENT_MAX_CHANNELS feature channels"};
  const int rc = kAffine ? check_window_args(who, total_rows, B, window, extents_ok, {many}, row_chunks,
                                             {src, starts, params, scale, shift, dst}, &st)
                         : check_window_args(who, total_rows, B, window, extents_ok, {many}, row_chunks,
                                             {src, starts, params, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  ChannelTable table;
  if (const int bad = fill_channel_table(who, channel_table, channels, &table)) return bad;
  hipLaunchKernelGGL(gather_augment_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), reinterpret_cast<const uint4*>(src), static_cast<long>(total_rows),
                     channels, freq_channels, starts, params, static_cast<long>(B), static_cast<int>(window), table,
                     mask_bits(mask_value), reinterpret_cast<const uint4*>(scale), reinterpret_cast<const uint4*>(shift),
                     reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

// the two label entry points
template <bool kStep>
static int permute_mask(const char* who, const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                        const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream_) {
  const int64_t cells = static_cast<int64_t>(I) * J;
  DeviceState* st;
  const int rc = check_window_args(
      who, total_rows, B, window, I > 0 && J > 0 && cells <= 65536,
      {{J % 4 != 0, kErrUnsupported, "a quarter turn is a whole number of cells only when J % 4 == 0"},
       {cells % 8 != 0, kErrUnsupported, "I*J must be a multiple of 8 (16-byte rows)"}},
      cells / 8, {src, starts, params, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  hipLaunchKernelGGL(permute_mask_kernel<kStep>, window_grid(window * (cells / 8), B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), src, static_cast<long>(total_rows), I, J, starts, params,
                     static_cast<long>(B), static_cast<int>(window), reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace seld

extern "C" {

int seld_window_gather_augment(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                               const int32_t* params, int64_t B, int64_t window, const uint8_t* channel_table,
                               float mask_value, float* dst, void* stream_) {
  return seld::gather_augment<false>("seld_window_gather_augment", src, total_rows, channels, freq_channels, starts, params, B,
                                     window, channel_table, mask_value, nullptr, nullptr, dst, stream_);
}

int seld_window_gather_augment_affine(const float* src, int64_t total_rows, int channels, int freq_channels,
                                      const int64_t* starts, const int32_t* params, int64_t B, int64_t window,
                                      const uint8_t* channel_table, float mask_value, const float* scale,
                                      const float* shift, float* dst, void* stream_) {
  return seld::gather_augment<true>("seld_window_gather_augment_affine", src, total_rows, channels, freq_channels, starts,
                                    params, B, window, channel_table, mask_value, scale, shift, dst, stream_);
}

int seld_window_permute_mask(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                             const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream_) {
  return seld::permute_mask<false>("seld_window_permute_mask", src, total_rows, I, J, starts, params, B, window, dst, stream_);
}

int seld_window_permute_mask_rotate(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                                    const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream_) {
  return seld::permute_mask<true>("seld_window_permute_mask_rotate", src, total_rows, I, J, starts, params, B, window, dst,
                                  stream_);
}

}  // extern "C"
