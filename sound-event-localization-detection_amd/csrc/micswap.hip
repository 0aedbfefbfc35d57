// Channel-swap augmentation of microphone-array features inside the device window gather for gfx950.
//
// A spatial pattern that maps the array onto itself is a permutation sigma of the microphones: the transformed scene's
// channel j is the recording's channel sigma(j).  The stored features follow, but not as plain channel copies:
//   * a log-mel channel c < C is the stored channel sigma(c);
//   * the GCC-PHAT channel of the pair (a, b) is the stored pair (sigma(a), sigma(b)) when that is in order, else the stored
//     pair (sigma(b), sigma(a)) with its lag axis reversed: out[j] = in[64 - j], j = 1..63, out[0] = in[0] (lag +32 is not
//     stored, so the -32 slot keeps its value);
//   * the NIPD channel m (reference microphone 0) is N(sigma(m)) - N(sigma(0)), N(0) = +0.0f, one fp32 subtraction; a
//     plain copy when the reference stays.
// The host turns sigma into one two-byte operation per (pattern, output channel), passed BY VALUE in the kernel arguments; a
// pattern that is no symmetry of the array carries identity operations.  Then, as in gather_augment_kernel: the affine
// map of the standardising export, the time / frequency masks, zero rows outside the timeline.
//
// One 16-byte store per thread and iteration, no LDS, no scratch, no atomics; blockIdx.y walks the windows.  A wavefront
// covers ONE output channel over four consecutive frames (4 x 16 chunks), so the channel's operation is a wave-uniform
// scalar load of the argument table and the choice between copy / reversed copy / difference a uniform branch.
#include "augment_core.h"

namespace seld {

constexpr int kMicMin = 2, kMicMax = 8;
constexpr int kMicMaxChannels = kMicMax + kMicMax * (kMicMax - 1) / 2;        // 36: 8 log-mel + 28 GCC-PHAT pairs
constexpr int kFramesPerWave = 64 / kChunksPerChannel;                        // 4

// One operation: bits 0..5 source channel a, bit 6 a's lag axis reversed, bit 7 a is the constant +0.0 (N(0));
// bits 8..15 source channel b that is SUBTRACTED, kNoSubtrahend for none.
constexpr unsigned kOpReversed = 0x40u, kOpZero = 0x80u, kNoSubtrahend = 0xffu;

// two operations per 32-bit word (channel c in half c & 1 of word c >> 1): there is no 16-bit scalar load
struct alignas(8) MicOps {
  uint32_t e[kPatterns][kMicMaxChannels / 2];
};

__device__ __forceinline__ uint4 minus(uint4 x, uint4 y) {
  return make_uint4(__float_as_uint(__uint_as_float(x.x) - __uint_as_float(y.x)),
                    __float_as_uint(__uint_as_float(x.y) - __uint_as_float(y.y)),
                    __float_as_uint(__uint_as_float(x.z) - __uint_as_float(y.z)),
                    __float_as_uint(__uint_as_float(x.w) - __uint_as_float(y.w)));
}

// dst[b][w][c][.] = operation (params[b] pattern, c) on row starts[b] + w of src, then scale / shift (kAffine), then masks
template <bool kAffine>
__global__ void __launch_bounds__(256)
gather_mic_kernel(const uint4* __restrict__ src, long total_rows, int channels, int freq_channels,
                  const int64_t* __restrict__ starts, const int32_t* __restrict__ params, long B, int window,
                  const MicOps ops, unsigned mask_bits, const uint4* __restrict__ scale, const uint4* __restrict__ shift,
                  uint4* __restrict__ dst) {
  const int row_chunks = channels * kChunksPerChannel;
  const int per_window = window * row_chunks;                       // host: < 2^31
  const int units = ((window + kFramesPerWave - 1) / kFramesPerWave) * channels;   // (four frames, channel) per wavefront
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int fr = lane / kChunksPerChannel, fc = lane % kChunksPerChannel;
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    for (int unit = blockIdx.x * 4 + wave; unit < units; unit += gridDim.x * 4) {
      // the quotient comes out of the vector unit: said to be uniform, so c is scalar and the table read a scalar load
      const int group = __builtin_amdgcn_readfirstlane(unit / channels);
      const int c = unit - group * channels;                        // < channels <= kMicMaxChannels
      const unsigned op = (ops.e[prm.pattern][c >> 1] >> (16 * (c & 1))) & 0xffffu;
      const int w = group * kFramesPerWave + fr;
      if (w >= window) continue;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        const uint4* __restrict__ row = src + srow * row_chunks;
        const uint4* __restrict__ a = row + (op & 0x3fu) * kChunksPerChannel;     // host: source channels < channels
        const unsigned sub = op >> 8;
        if (sub != kNoSubtrahend) {                                 // NIPD with a moved reference: N(a) - N(b)
          const uint4 x = (op & kOpZero) ? make_uint4(0u, 0u, 0u, 0u) : a[fc];
          v = minus(x, row[sub * kChunksPerChannel + fc]);
        } else if (op & kOpReversed) {                              // GCC-PHAT pair out of order: the lag axis turned round
          const uint4 head = a[fc == 0 ? 0 : kChunksPerChannel - fc];
          const uint4 tail = a[kChunksPerChannel - 1 - fc];
          v = make_uint4(head.x, tail.w, tail.z, tail.y);
        } else {
          v = a[fc];
        }
        v = standardised<kAffine>(v, scale, shift, c * kChunksPerChannel + fc);
        v = masked(v, w, c, fc, prm, freq_channels, mask_bits);
      }
      to[w * row_chunks + c * kChunksPerChannel + fc] = v;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static inline int mic_channels(int mics, int kind) {
  return kind == SELD_MIC_GCC ? mics + mics * (mics - 1) / 2 : 2 * mics - 1;
}

// 0: row is a permutation of 0..mics-1; 1: all -1 (no symmetry of this array); -1: neither
static int classify_row(const int8_t* row, int mics) {
  bool none = true;
  for (int j = 0; j < mics; ++j) none = none && row[j] == -1;
  if (none) return 1;
  unsigned seen = 0;
  for (int j = 0; j < mics; ++j) {
    if (row[j] < 0 || row[j] >= mics || (seen >> row[j]) & 1u) return -1;
    seen |= 1u << row[j];
  }
  return 0;
}

static bool table_rows_ok(const int8_t* mic_perm, int mics) {
  for (int p = 0; p < kPatterns; ++p)
    if (classify_row(mic_perm + p * mics, mics) < 0) return false;
  return true;
}

static bool first_row_is_identity(const int8_t* mic_perm, int mics) {
  for (int j = 0; j < mics; ++j)
    if (mic_perm[j] != j) return false;
  return true;
}

// the operations of every (pattern, output channel) from the checked permutation table
static void fill_ops(const int8_t* mic_perm, int mics, int kind, MicOps* ops) {
  const int C = mics;
  const unsigned none = kNoSubtrahend << 8;
  auto pair_channel = [C](int a, int b) { return C + a * C - a * (a + 1) / 2 + (b - a - 1); };      // a < b, lexicographic
  for (int p = 0; p < kPatterns; ++p) {
    unsigned e[kMicMaxChannels];
    for (int c = 0; c < kMicMaxChannels; ++c) e[c] = none | (c < mic_channels(C, kind) ? c : 0);
    const int8_t* s = mic_perm + p * C;
    if (classify_row(s, C) == 0) {                                  // (not a symmetry: the identity stays)
      for (int c = 0; c < C; ++c) e[c] = none | s[c];
      if (kind == SELD_MIC_GCC) {
        for (int a = 0; a < C; ++a)
          for (int b = a + 1; b < C; ++b) {
            const int u = s[a], v = s[b];
            e[pair_channel(a, b)] = u < v ? none | pair_channel(u, v) : none | kOpReversed | pair_channel(v, u);
          }
      } else {
        for (int m = 1; m < C; ++m) {
          const int sm = s[m], s0 = s[0];
          if (s0 == 0) e[C + m - 1] = none | (C + sm - 1);
          else e[C + m - 1] = (static_cast<unsigned>(C + s0 - 1) << 8) | (sm == 0 ? kOpZero : C + sm - 1);
        }
      }
    }
    for (int c = 0; c < kMicMaxChannels; c += 2) ops->e[p][c / 2] = (e[c] & 0xffffu) | (e[c + 1] << 16);
  }
}

template <bool kAffine>
static int gather_mic(const char* who, const float* src, int64_t total_rows, int mics, int kind, int freq_channels,
                      const int64_t* starts, const int32_t* params, int64_t B, int64_t window, const int8_t* mic_perm,
                      float mask_value, const float* scale, const float* shift, float* dst, void* stream_) {
  DeviceState* st;
  const bool mics_ok = mics >= kMicMin && mics <= kMicMax;
  const bool kind_ok = kind == SELD_MIC_GCC || kind == SELD_MIC_NIPD;
  const int channels = mics_ok && kind_ok ? mic_channels(mics, kind) : 0;
  const bool extents_ok = mics_ok && kind_ok && freq_channels >= 0 && freq_channels <= channels;
  const int64_t row_chunks = static_cast<int64_t>(channels) * kChunksPerChannel;
  // the table is read here only when the extents hold; a NULL one is refused with the other pointers
  const bool readable = extents_ok && mic_perm != nullptr;
  const Refusal rows{readable && !table_rows_ok(mic_perm, mics), kErrInvalidArgument,
                     "a mic_perm row is neither a permutation of the microphones nor all -1"};
  const Refusal first{readable && !first_row_is_identity(mic_perm, mics), kErrInvalidArgument,
                      "mic_perm row 0 (pattern 0) must be the identity"};
  const int rc = kAffine ? check_window_args(who, total_rows, B, window, extents_ok, {rows, first}, row_chunks,
                                             {src, starts, params, mic_perm, scale, shift, dst}, &st)
                         : check_window_args(who, total_rows, B, window, extents_ok, {rows, first}, row_chunks,
                                             {src, starts, params, mic_perm, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  MicOps ops;
  fill_ops(mic_perm, mics, kind, &ops);
  const long units = (window + kFramesPerWave - 1) / kFramesPerWave * channels;
  hipLaunchKernelGGL(gather_mic_kernel<kAffine>, window_grid(units * 64, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), reinterpret_cast<const uint4*>(src), static_cast<long>(total_rows),
                     channels, freq_channels, starts, params, static_cast<long>(B), static_cast<int>(window), ops,
                     mask_bits(mask_value), reinterpret_cast<const uint4*>(scale), reinterpret_cast<const uint4*>(shift),
                     reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace seld

extern "C" {

int seld_window_gather_mic(const float* src, int64_t total_rows, int mics, int kind, int freq_channels, const int64_t* starts,
                           const int32_t* params, int64_t B, int64_t window, const int8_t* mic_perm, float mask_value,
                           float* dst, void* stream_) {
  return seld::gather_mic<false>("seld_window_gather_mic", src, total_rows, mics, kind, freq_channels, starts, params, B,
                                 window, mic_perm, mask_value, nullptr, nullptr, dst, stream_);
}

int seld_window_gather_mic_standardised(const float* src, int64_t total_rows, int mics, int kind, int freq_channels,
                                  const int64_t* starts, const int32_t* params, int64_t B, int64_t window,
                                  const int8_t* mic_perm, float mask_value, const float* scale, const float* shift,
                                  float* dst, void* stream_) {
  return seld::gather_mic<true>("seld_window_gather_mic_standardised", src, total_rows, mics, kind, freq_channels, starts, params,
                                B, window, mic_perm, mask_value, scale, shift, dst, stream_);
}

}  // extern "C"
