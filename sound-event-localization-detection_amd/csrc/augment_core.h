// What the window gathers share (labels.hip: the plain gather; augment.hip: the 16 sign-and-swap transforms and the label
// permutation; rotate.hip: the same features with azimuth steps): the per-window parameter row, the mask test, the signed
// channel copy, the standardising map of their kAffine instantiations, the by-value channel table, the launch grid and the
// host prologue of the eight entry points.
//
// The two feature kernels stay two kernels: gather_rotate_kernel walks units, takes three by-value tables and needs 44
// VGPRs against gather_augment_kernel's 16, so folding them would make the default training path pay for the rotating one.
// They share the helpers below and nothing more.
#pragma once

#include <initializer_list>

#include "seld_common.h"

#include "seld_hip.h"

namespace seld {

constexpr int kParamInts = SELD_AUGMENT_PARAM_INTS;
constexpr int kPatterns = SELD_AUGMENT_PATTERNS;
constexpr int kMaxChannels = SELD_AUGMENT_MAX_CHANNELS;
constexpr int kFeatureBins = 64;                    // mel bins (or GCC-PHAT lags) per feature channel
constexpr int kChunksPerChannel = kFeatureBins / 4; // 16-byte chunks of one channel row

struct WindowParams {
  int pattern, t0, tl0, t1, tl1, f0, fl0, f1, fl1;
};

__device__ __forceinline__ WindowParams load_params(const int32_t* __restrict__ params, long b) {
  const int32_t* row = params + b * kParamInts;
  WindowParams w;
  w.pattern = row[0] & (kPatterns - 1);
  w.t0 = row[1]; w.tl0 = row[2]; w.t1 = row[3]; w.tl1 = row[4];
  w.f0 = row[5]; w.fl0 = row[6]; w.f1 = row[7]; w.fl1 = row[8];
  return w;
}

// x in [start, start + len) without forming start + len; the distance is taken in unsigned arithmetic, where it cannot
// overflow whatever a hostile row holds
__device__ __forceinline__ bool in_span(int x, int start, int len) {
  return len > 0 && x >= start && static_cast<unsigned>(x) - static_cast<unsigned>(start) < static_cast<unsigned>(len);
}

// row[9] reduced to 0..J-1 whatever it holds
__device__ __forceinline__ int azimuth_step(const int32_t* __restrict__ params, long b, int J) {
  const int r = params[b * kParamInts + 9] % J;
  return r < 0 ? r + J : r;
}

// (source channel | 0x80 when negated) of every output channel, per pattern: passed BY VALUE (kernel argument memory).
// gather_augment_kernel takes all kMaxChannels columns, gather_rotate_kernel (4 or 7 channels) only 8.
template <int kColumns>
struct alignas(8) ChannelTableOf {
  uint8_t e[kPatterns][kColumns];
};
using ChannelTable = ChannelTableOf<kMaxChannels>;
using ChannelTable8 = ChannelTableOf<8>;

// byte c of a table row of up to 8 channels held in one register pair
__device__ __forceinline__ unsigned packed_entry(unsigned long long packed, unsigned c) {
  return static_cast<unsigned>(packed >> (8 * c)) & 0xffu;
}

// 16 bytes of the source channel a table entry names, negated when the entry says so; row: one frame of the timeline
__device__ __forceinline__ uint4 signed_copy(const uint4* __restrict__ row, unsigned entry, int fc) {
  const unsigned flip = (entry & 0x80u) << 24;                      // sign bit
  uint4 v = row[(entry & 0x7fu) * kChunksPerChannel + fc];          // host: source channel < channels
  v.x ^= flip; v.y ^= flip; v.z ^= flip; v.w ^= flip;
  return v;
}

// The standardising instantiations of the three feature kernels (kAffine): fmaf(v, scale, shift) on the
// four floats of a chunk, `entry` the chunk's place in the [channels][64] tables = output channel * kChunksPerChannel + fc.
// Two 16-byte loads of tables that stay in cache (at most 18 KB); called in front of masked(), so a masked element is
// exactly the mask value.  The other instantiation is the kernel as it was: nothing is loaded and v comes back untouched.
template <bool kAffine>
__device__ __forceinline__ uint4 standardised(uint4 v, const uint4* __restrict__ scale, const uint4* __restrict__ shift,
                                              int entry) {
  if constexpr (kAffine) {
    const uint4 s = scale[entry], b = shift[entry];
    v.x = __float_as_uint(fmaf(__uint_as_float(v.x), __uint_as_float(s.x), __uint_as_float(b.x)));
    v.y = __float_as_uint(fmaf(__uint_as_float(v.y), __uint_as_float(s.y), __uint_as_float(b.y)));
    v.z = __float_as_uint(fmaf(__uint_as_float(v.z), __uint_as_float(s.z), __uint_as_float(b.z)));
    v.w = __float_as_uint(fmaf(__uint_as_float(v.w), __uint_as_float(s.w), __uint_as_float(b.w)));
  }
  return v;
}

// the time / frequency masks on one 16-byte chunk (bins 4 fc .. 4 fc + 3) of frame w of output channel c
__device__ __forceinline__ uint4 masked(uint4 v, int w, int c, int fc, const WindowParams& prm, int freq_channels,
                                        unsigned mask_bits) {
  if (in_span(w, prm.t0, prm.tl0) || in_span(w, prm.t1, prm.tl1)) return make_uint4(mask_bits, mask_bits, mask_bits, mask_bits);
  if (c < freq_channels) {
    const int f = fc * 4;
    if (in_span(f + 0, prm.f0, prm.fl0) || in_span(f + 0, prm.f1, prm.fl1)) v.x = mask_bits;
    if (in_span(f + 1, prm.f0, prm.fl0) || in_span(f + 1, prm.f1, prm.fl1)) v.y = mask_bits;
    if (in_span(f + 2, prm.f0, prm.fl0) || in_span(f + 2, prm.f1, prm.fl1)) v.z = mask_bits;
    if (in_span(f + 3, prm.f0, prm.fl0) || in_span(f + 3, prm.f1, prm.fl1)) v.w = mask_bits;
  }
  return v;
}

// The partner of window b in the mixing gathers (mix.hip): row b of int64 [B][2] =
// (start frame sb, fp32 bits of the linear power gain g in bits 0..31 | spatial pattern pb in bits 32..35).  A gain that is
// not a finite value > 0 (0, negative, NaN, infinity) means NO partner, whatever the other fields hold.  As with a parameter
// row nothing is trusted: the pattern is reduced modulo 16, the start only goes through the row-in-timeline test, the gain
// is only multiplied.
struct Partner {
  long start;
  float gain;
  int pattern;
  bool on;
};

__device__ __forceinline__ Partner load_partner(const int64_t* __restrict__ partners, long b) {
  Partner p;
  p.start = partners[2 * b];
  const unsigned long long packed = static_cast<unsigned long long>(partners[2 * b + 1]);
  p.gain = __uint_as_float(static_cast<unsigned>(packed));
  p.pattern = static_cast<int>(packed >> 32) & (kPatterns - 1);
  p.on = p.gain > 0.0f && p.gain < __builtin_huge_valf();            // a NaN fails both comparisons
  return p;
}

// The spectral row of window b in the in-place stage (spectral.hip): int32 x SELD_SPECTRAL_PARAM_INTS =
// [0] frequency shift s, [1] flags (bit 0: the window has a gain curve), [2..5] / [6..9] two cutouts (t, tl, f0, fl).  Nothing
// is trusted: the shift is clamped to +-64 (beyond +-63 every bin is an edge copy anyway) and then only selects a bin through
// a second clamp, the cutout fields are only compared.
constexpr int kSpectralInts = SELD_SPECTRAL_PARAM_INTS;

struct SpectralParams {
  int shift;
  bool curve;
  int t0, tl0, f0, fl0, t1, tl1, f1, fl1;
};

__device__ __forceinline__ SpectralParams load_spectral(const int32_t* __restrict__ spectral, long b) {
  const int32_t* row = spectral + b * kSpectralInts;
  SpectralParams s;
  s.shift = row[0] < -kFeatureBins ? -kFeatureBins : row[0] > kFeatureBins ? kFeatureBins : row[0];
  s.curve = (row[1] & 1) != 0;
  s.t0 = row[2]; s.tl0 = row[3]; s.f0 = row[4]; s.fl0 = row[5];
  s.t1 = row[6]; s.tl1 = row[7]; s.f1 = row[8]; s.fl1 = row[9];
  return s;
}

// neither cutout of the row can hit an element
__device__ __forceinline__ bool no_cutouts(const SpectralParams& s) {
  return (s.tl0 <= 0 || s.fl0 <= 0) && (s.tl1 <= 0 || s.fl1 <= 0);
}

// the two cutout rectangles on one 16-byte chunk (bins 4 fc .. 4 fc + 3) of frame w of output channel c
__device__ __forceinline__ uint4 cut_out(uint4 v, int w, int c, int fc, const SpectralParams& s, int freq_channels,
                                         unsigned mask_bits) {
  if (c >= freq_channels) return v;
  const bool in0 = in_span(w, s.t0, s.tl0), in1 = in_span(w, s.t1, s.tl1);
  const int f = fc * 4;
  if ((in0 && in_span(f + 0, s.f0, s.fl0)) || (in1 && in_span(f + 0, s.f1, s.fl1))) v.x = mask_bits;
  if ((in0 && in_span(f + 1, s.f0, s.fl0)) || (in1 && in_span(f + 1, s.f1, s.fl1))) v.y = mask_bits;
  if ((in0 && in_span(f + 2, s.f0, s.fl0)) || (in1 && in_span(f + 2, s.f1, s.fl1))) v.z = mask_bits;
  if ((in0 && in_span(f + 3, s.f0, s.fl0)) || (in1 && in_span(f + 3, s.f1, s.fl1))) v.w = mask_bits;
  return v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static inline unsigned mask_bits(float mask_value) {
  unsigned bits;
  static_assert(sizeof(bits) == sizeof(mask_value), "fp32 bit pattern");
  __builtin_memcpy(&bits, &mask_value, sizeof(bits));
  return bits;
}

// The by-value table from the host's uint8 [kPatterns][channels] array; NULL: every pattern is the identity (an entry point
// that does not allow NULL refuses it with its other pointers).  Columns >= channels are zero and never read.
template <int kColumns>
inline int fill_channel_table(const char* who, const uint8_t* channel_table, int channels, ChannelTableOf<kColumns>* table) {
  for (int p = 0; p < kPatterns; ++p)
    for (int c = 0; c < kColumns; ++c) {
      uint8_t e = static_cast<uint8_t>(c < channels ? c : 0);
      if (channel_table && c < channels) {
        e = channel_table[p * channels + c];
        if ((e & 0x7f) >= channels)
          return fail(kErrInvalidArgument, std::string(who) + ": channel table names a channel >= channels");
      }
      table->e[p][c] = e;
    }
  return kOk;
}

static inline dim3 window_grid(long per_window, long B, int num_cus) {
  long x = (per_window + 255) / 256;
  const long cap = static_cast<long>(num_cus) * 32;
  long y = B < 65535 ? B : 65535;
  if (x * y > cap) x = (cap + y - 1) / y;                           // grid-stride over the window's chunks
  if (x < 1) x = 1;
  return dim3(static_cast<unsigned>(x), static_cast<unsigned>(y));
}

// ---- the host prologue of the eight entry points ---------------------------------------------------------------------------
struct Refusal {        // one of an entry point's own conditions: refused with `code` and "<entry point>: <why>" when `hit`
  bool hit;
  int code;
  const char* why;
};

// In this order: the library's state, the extents (total_rows, B, window and `extents_ok`, the entry point's own), the entry
// point's own refusals in the order given, the chunks of one window (`frame_chunks` 16-byte chunks per frame; 0: the kernel
// indexes in 64 bits and there is no limit), the empty call -- before any pointer is looked at -- and the pointers.  Returns
// kOk with *state set; a caller launches nothing when the code is not kOk or B is 0.
inline int check_window_args(const char* who, int64_t total_rows, int64_t B, int64_t window, bool extents_ok,
                             std::initializer_list<Refusal> own, int64_t frame_chunks,
                             std::initializer_list<const void*> pointers, DeviceState** state) {
  const std::string name(who);
  *state = current_state();
  if (!*state) return kErrNotInitialised;
  if (total_rows < 0 || B < 0 || window <= 0 || !extents_ok) return fail(kErrInvalidArgument, name + ": bad extents");
  for (const Refusal& r : own)
    if (r.hit) return fail(r.code, name + ": " + r.why);
  // window * frame_chunks >= 2^31, without forming the product
  if (frame_chunks > 0 && window > ((int64_t{1} << 31) - 1) / frame_chunks) return fail(kErrUnsupported, name + ": window too large");
  if (B == 0) return kOk;
  for (const void* ptr : pointers)
    if (!ptr) return fail(kErrInvalidArgument, name + ": null pointer");
  return kOk;
}

}  // namespace seld
