// Frequency shift, gain curve and cutouts as ONE in-place stage on a gathered batch, for gfx950.
//
// Every feature gather writes float32 [B][window][channels][64] into the static input buffer of the captured step.  This
// stage rewrites that buffer where it stands, per window b from its spectral row (augment_core.h), per element in this order:
//   1. row starts[b] + w outside the timeline: untouched (the gather's zeros);
//   2. c < freq_channels: v = x[clamp(f - s, 0, 63)] (edge replication), else v = x[f];
//   3. c < logmel_channels and the window has a curve: v <= -100 stays, else v = max(v + G[b][f], -100);
//   4. kAffine: v = fmaf(v, scale[c][f], shift[c][f])                     (standardised<true>, the arithmetic of section 22);
//   5. the masks of the window's parameter row (masked()), then the two cutouts (cut_out()).
//
// In place and race-free by construction.  A thread owns 16-byte chunks: the only loads of the batch it issues are of chunks
// it then stores (or, in a row outside the timeline, leaves alone), to the same addresses.  The 16 chunks of one 256-byte (frame, channel) row sit in 16 consecutive lanes of one wavefront -- the
// block size, the grid stride and the chunks of a window are all multiples of 16 -- so the shift, the only step that reads a
// bin other than the one it writes, takes its bins from the REGISTERS of those lanes (__shfl of width 16 = ds_bpermute_b32).
// No lane ever reads an address another lane writes; there is no ordering between loads and stores to rely on.
// For s = 4 q + r the four source bins of a lane's chunk lie in the chunks of lanes -q and -q - 1: output element j is
// element (j - s) & 3, the same in every lane (a rotation of the chunk on a scalar condition), of lane (4 fc + j - s) >> 2,
// clamped to the row; a bin that falls off the row is the row's bin 0 or bin 63 instead, fetched from lanes 0 and 15.  Six
// cross-lane moves per chunk, none when s = 0.
//
// 16-byte loads and stores only, no LDS allocation, no scratch, no atomics.  blockIdx.y walks the windows, so both rows of a
// window, its start and its flags are wave-uniform; its curve is one 256-byte row that stays in cache.  A window with nothing
// to do (identity spectral row, no masks, no map) is skipped whole: neither read nor written.
#include "augment_core.h"

namespace seld {

constexpr float kSpectralFloor = -100.0f;               // power_to_db's floor: a stored value at or below it is power 0

// the chunk's elements rotated left by r (wave-uniform, 0..3): element j of the result is element (j + r) & 3 of v.  Two
// rounds of selects on a scalar condition; no register array is indexed
__device__ __forceinline__ uint4 rotated(const uint4& v, int r) {
  const uint4 a = (r & 1) ? make_uint4(v.y, v.z, v.w, v.x) : v;
  return (r & 2) ? make_uint4(a.z, a.w, a.x, a.y) : a;
}

// bins 4 fc .. 4 fc + 3 of the row shifted by s (wave-uniform, |s| <= 64, s != 0); v: this lane's own chunk.  Every lane of the
// wavefront calls this, whether its row is live or not.
__device__ __forceinline__ uint4 shifted_chunk(const uint4& v, int fc, int s) {
  constexpr int kRow = kChunksPerChannel;               // lanes per row
  const unsigned first = __shfl(v.x, 0, kRow), last = __shfl(v.w, kRow - 1, kRow);
  const uint4 e = rotated(v, -s & 3);                   // e.j = element (j - s) & 3: what output element j takes from its lane
  const int bin = 4 * fc - s;                           // source bin of output element 0: -64 .. 124
  const auto pick = [&](unsigned mine, int at) {
    const int lane = at < 0 ? 0 : at >= kFeatureBins ? kRow - 1 : at >> 2;
    const unsigned got = __shfl(mine, lane, kRow);
    return at < 0 ? first : at >= kFeatureBins ? last : got;
  };
  return make_uint4(pick(e.x, bin), pick(e.y, bin + 1), pick(e.z, bin + 2), pick(e.w, bin + 3));
}

// v <= -100 stays; else max(v + g, -100): one fp32 addition
__device__ __forceinline__ unsigned gained(unsigned bits, float g) {
  const float v = __uint_as_float(bits);
  return v <= kSpectralFloor ? bits : __float_as_uint(fmaxf(__fadd_rn(v, g), kSpectralFloor));
}

template <bool kAffine>
__global__ void __launch_bounds__(256)
spectral_kernel(uint4* batch, long total_rows, int channels, int logmel_channels, int freq_channels,
                const int64_t* __restrict__ starts, const int32_t* __restrict__ params, const int32_t* __restrict__ spectral,
                const float* __restrict__ curves, long B, int window, unsigned mask_bits, const uint4* __restrict__ scale,
                const uint4* __restrict__ shift) {
  const int row_chunks = channels * kChunksPerChannel;
  const int per_window = window * row_chunks;                       // host: < 2^31; a multiple of 16
  const int lane = threadIdx.x & 63;
  const long stride = static_cast<long>(gridDim.x) * blockDim.x;
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const SpectralParams sp = load_spectral(spectral, b);
    WindowParams prm{};
    if (params) prm = load_params(params, b);
    const bool curve = sp.curve && curves != nullptr && logmel_channels > 0;
    const bool masks = prm.tl0 > 0 || prm.tl1 > 0 || prm.fl0 > 0 || prm.fl1 > 0;
    if (!kAffine && sp.shift == 0 && !curve && !masks && no_cutouts(sp)) continue;      // nothing to do: not rewritten
    const long start = starts[b];
    uint4* own = batch + b * static_cast<long>(per_window);
    const uint4* __restrict__ gains = curve ? reinterpret_cast<const uint4*>(curves) + b * kChunksPerChannel : nullptr;
    const int fc = lane & (kChunksPerChannel - 1);                  // row_chunks, blockDim and the stride are multiples of 16
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    // The curve chunk and the lane's first chunk are requested before anything is computed, and inside the loop the NEXT
    // chunk before the current one is worked on: an address needs no division, and a row outside the timeline may be read
    // (it lies in the batch), only not written.  Still the only loads of the batch: chunks this lane stores or skips.
    uint4 g = zero;
    if (curve) g = gains[fc];
    // wave-uniform trip count: the cross-lane moves are executed by whole wavefronts
    long q0 = static_cast<long>(blockIdx.x) * blockDim.x + (threadIdx.x - lane);
    uint4 ahead = zero;
    if (q0 + lane < per_window) ahead = own[q0 + lane];
    for (; q0 < per_window; q0 += stride) {
      const long q = q0 + lane;
      const bool inside = q < per_window;                           // the same for the 16 lanes of a row
      const int qi = static_cast<int>(inside ? q : 0);
      uint4 v = ahead;
      if (q + stride < per_window) ahead = own[q + stride];
      const int w = qi / row_chunks;
      const int chunk = qi - w * row_chunks;
      const int c = chunk / kChunksPerChannel;
      const long srow = start + w;
      const bool live = inside && srow >= 0 && srow < total_rows;   // the same for the 16 lanes of a row
      if (sp.shift != 0) {
        const uint4 moved = shifted_chunk(v, fc, sp.shift);
        if (c < freq_channels) v = moved;
      }
      if (!live) continue;
      if (curve && c < logmel_channels) {
        v.x = gained(v.x, __uint_as_float(g.x)); v.y = gained(v.y, __uint_as_float(g.y));
        v.z = gained(v.z, __uint_as_float(g.z)); v.w = gained(v.w, __uint_as_float(g.w));
      }
      v = standardised<kAffine>(v, scale, shift, chunk);
      v = masked(v, w, c, fc, prm, freq_channels, mask_bits);
      v = cut_out(v, w, c, fc, sp, freq_channels, mask_bits);
      own[qi] = v;
    }
  }
}

template <bool kAffine>
static int window_spectral(const char* who, float* batch, int64_t total_rows, int channels, int logmel_channels,
                           int freq_channels, const int64_t* starts, const int32_t* params, const int32_t* spectral,
                           const float* curves, int64_t B, int64_t window, float mask_value, const float* scale,
                           const float* shift, void* stream_) {
  DeviceState* st;
  const int64_t row_chunks = static_cast<int64_t>(channels) * kChunksPerChannel;
  const bool extents_ok = channels > 0 && logmel_channels >= 0 && logmel_channels <= freq_channels && freq_channels <= channels;
  const int rc = kAffine ? check_window_args(who, total_rows, B, window, extents_ok, {}, row_chunks,
                                             {batch, starts, spectral, scale, shift}, &st)
                         : check_window_args(who, total_rows, B, window, extents_ok, {}, row_chunks, {batch, starts, spectral},
                                             &st);
  if (rc != kOk || B == 0) return rc;
  hipLaunchKernelGGL(spectral_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), reinterpret_cast<uint4*>(batch), static_cast<long>(total_rows), channels,
                     logmel_channels, freq_channels, starts, params, spectral, curves, static_cast<long>(B),
                     static_cast<int>(window), mask_bits(mask_value), reinterpret_cast<const uint4*>(scale),
                     reinterpret_cast<const uint4*>(shift));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace seld

extern "C" {

int seld_window_spectral(float* batch, int64_t total_rows, int channels, int logmel_channels, int freq_channels,
                         const int64_t* starts, const int32_t* params, const int32_t* spectral, const float* curves, int64_t B,
                         int64_t window, float mask_value, void* stream_) {
  return seld::window_spectral<false>("seld_window_spectral", batch, total_rows, channels, logmel_channels, freq_channels, starts,
                                      params, spectral, curves, B, window, mask_value, nullptr, nullptr, stream_);
}

int seld_window_spectral_standardised(float* batch, int64_t total_rows, int channels, int logmel_channels, int freq_channels,
                                      const int64_t* starts, const int32_t* params, const int32_t* spectral,
                                      const float* curves, int64_t B, int64_t window, float mask_value, const float* scale,
                                      const float* shift, void* stream_) {
  return seld::window_spectral<true>("seld_window_spectral_standardised", batch, total_rows, channels, logmel_channels,
                                     freq_channels, starts, params, spectral, curves, B, window, mask_value, scale, shift,
                                     stream_);
}

}  // extern "C"
