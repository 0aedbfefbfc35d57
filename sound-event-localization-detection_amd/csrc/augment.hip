// Training augmentation inside the device window gather for gfx950 -- pure data movement, bit-exact.
//
// The plain gather (labels.hip, gather_rows_kernel) copies 250-frame windows from the device timeline into the static
// input buffers of a captured step.  These two kernels do the same copy and, on the way, apply per window
//   * one of the 16 sign-and-swap transforms of the first-order-Ambisonics channels: an exact signed
//     permutation of the feature channels and an exact permutation of the DOA grid cells, and
//   * up to two time masks and two frequency masks (SpecAugment) on the features.
// The transform of window b is row b of a parameter table in device memory (SELD_AUGMENT_PARAM_INTS int32 per row):
//   [0] pattern p (0..15; 0 = identity): mirror m = p >> 3, then k = (p >> 1) & 3 quarter turns, then elevation flip e = p & 1
//   [1] [2] time mask 0: first frame, length      [3] [4] time mask 1
//   [5] [6] frequency mask 0: first bin, length   [7] [8] frequency mask 1
//   [9..11] padding (ignored)
// A row is trusted no further than its bits: the pattern is reduced modulo 16 and the masks are only ever COMPARED with
// the coordinates the kernel itself generates, so no parameter value can move a load or a store.
//
// Both kernels: one 16-byte store per thread and iteration, no LDS, no scratch, no atomics; blockIdx.y walks the windows,
// so a window's parameter row and start frame are wave-uniform (scalar loads).  The output of a window depends on
// (source, starts[b], params[b]) only.
#include "augment_core.h"

namespace seld {

// (source channel | 0x80 when negated) of every output channel, per pattern: passed BY VALUE (kernel argument memory).
struct alignas(8) ChannelTable {
  uint8_t e[kPatterns][kMaxChannels];
};

// dst[b][w][c][f] = sign * src[starts[b] + w][srcch[c]][f], then the masks; rows past the timeline stay zero.
__global__ void __launch_bounds__(256)
gather_augment_kernel(const uint4* __restrict__ src, long total_rows, int channels, int freq_channels,
                      const int64_t* __restrict__ starts, const int32_t* __restrict__ params, long B, int window,
                      const ChannelTable table, unsigned mask_bits, uint4* __restrict__ dst) {
  const int row_chunks = channels * kChunksPerChannel;
  const int per_window = window * row_chunks;                       // host: < 2^31
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const long start = starts[b];
    const uint4* __restrict__ from = src;
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
        const unsigned entry = channels <= 8 ? static_cast<unsigned>(packed >> (8 * c)) & 0xffu : table.e[prm.pattern][c];
        const int sc = static_cast<int>(entry & 0x7fu);             // host: < channels
        const unsigned flip = (entry & 0x80u) << 24;                // sign bit
        v = from[srow * row_chunks + sc * kChunksPerChannel + fc];
        v.x ^= flip; v.y ^= flip; v.z ^= flip; v.w ^= flip;
        if (in_span(w, prm.t0, prm.tl0) || in_span(w, prm.t1, prm.tl1)) {
          v = make_uint4(mask_bits, mask_bits, mask_bits, mask_bits);
        } else if (c < freq_channels) {
          const int f = fc * 4;
          if (in_span(f + 0, prm.f0, prm.fl0) || in_span(f + 0, prm.f1, prm.fl1)) v.x = mask_bits;
          if (in_span(f + 1, prm.f0, prm.fl0) || in_span(f + 1, prm.f1, prm.fl1)) v.y = mask_bits;
          if (in_span(f + 2, prm.f0, prm.fl0) || in_span(f + 2, prm.f1, prm.fl1)) v.z = mask_bits;
          if (in_span(f + 3, prm.f0, prm.fl0) || in_span(f + 3, prm.f1, prm.fl1)) v.w = mask_bits;
        }
      }
      to[q] = v;
    }
  }
}

// dst[b][w][cell'] = src[starts[b] + w][cell], cell -> cell' the pattern's grid permutation: a set cell (i, j) moves to
//   i' = e ? I-1-i : i,   j' = ((m ? J-1-j : j) + k*J/4) mod J.
// Each thread builds 8 consecutive destination cells (one 16-byte store) from their source cells.  The identity pattern
// (and any pattern on a row past the timeline) keeps the 16-byte load of the plain gather; every other pattern reads 2-byte
// cells: J = 36 is not a multiple of 8, so a mirrored or rotated grid row has no 16-byte-aligned image in the source row.
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
    const int shift = ((p >> 1) & 3) * quarter;
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_chunks;
      const int chunk = q - w * row_chunks;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        const uint16_t* __restrict__ row = src + srow * cells;
        if (p == 0) {
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

}  // namespace seld

extern "C" {

int seld_window_gather_augment(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                               const int32_t* params, int64_t B, int64_t window, const uint8_t* channel_table,
                               float mask_value, float* dst, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (total_rows < 0 || B < 0 || window <= 0 || channels <= 0 || freq_channels < 0 || freq_channels > channels)
    return fail(kErrInvalidArgument, "seld_window_gather_augment: bad extents");
  if (channels > kMaxChannels)
    return fail(kErrUnsupported, "seld_window_gather_augment: more than SELD_AUGMENT_MAX_CHANNELS feature channels");
  if (window * channels * kChunksPerChannel >= (int64_t{1} << 31))
    return fail(kErrUnsupported, "seld_window_gather_augment: window too large");
  if (B == 0) return kOk;
  if (!src || !starts || !params || !dst) return fail(kErrInvalidArgument, "seld_window_gather_augment: null pointer");
  ChannelTable table;
  for (int p = 0; p < kPatterns; ++p)
    for (int c = 0; c < kMaxChannels; ++c) {
      uint8_t e = static_cast<uint8_t>(c < channels ? c : 0);       // NULL table: every pattern is the identity
      if (channel_table && c < channels) {
        e = channel_table[p * channels + c];
        if ((e & 0x7f) >= channels)
          return fail(kErrInvalidArgument, "seld_window_gather_augment: channel table names a channel >= channels");
      }
      table.e[p][c] = e;
    }
  unsigned mask_bits;
  static_assert(sizeof(mask_bits) == sizeof(mask_value), "fp32 bit pattern");
  __builtin_memcpy(&mask_bits, &mask_value, sizeof(mask_bits));
  const long per_window = window * channels * kChunksPerChannel;
  hipLaunchKernelGGL(gather_augment_kernel, window_grid(per_window, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), reinterpret_cast<const uint4*>(src), static_cast<long>(total_rows),
                     channels, freq_channels, starts, params, static_cast<long>(B), static_cast<int>(window), table,
                     mask_bits, reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_window_permute_mask(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts,
                             const int32_t* params, int64_t B, int64_t window, uint16_t* dst, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (total_rows < 0 || B < 0 || window <= 0 || I <= 0 || J <= 0 || static_cast<int64_t>(I) * J > 65536)
    return fail(kErrInvalidArgument, "seld_window_permute_mask: bad extents");
  if (J % 4 != 0)
    return fail(kErrUnsupported, "seld_window_permute_mask: a quarter turn is a whole number of cells only when J % 4 == 0");
  if ((I * J) % 8 != 0)
    return fail(kErrUnsupported, "seld_window_permute_mask: I*J must be a multiple of 8 (16-byte rows)");
  if (window * (I * J / 8) >= (int64_t{1} << 31))
    return fail(kErrUnsupported, "seld_window_permute_mask: window too large");
  if (B == 0) return kOk;
  if (!src || !starts || !params || !dst) return fail(kErrInvalidArgument, "seld_window_permute_mask: null pointer");
  const long per_window = window * (I * J / 8);
  hipLaunchKernelGGL(permute_mask_kernel, window_grid(per_window, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), src, static_cast<long>(total_rows), I, J, starts, params,
                     static_cast<long>(B), static_cast<int>(window), reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
