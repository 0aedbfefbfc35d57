// Device helpers shared by the augmenting window gathers (augment.hip: the 16 sign-and-swap transforms; rotate.hip: the
// same with azimuth steps): the per-window parameter row, the mask test and the launch grid.
#pragma once

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

static inline dim3 window_grid(long per_window, long B, int num_cus) {
  long x = (per_window + 255) / 256;
  const long cap = static_cast<long>(num_cus) * 32;
  long y = B < 65535 ? B : 65535;
  if (x * y > cap) x = (cap + y - 1) / y;                           // grid-stride over the window's chunks
  if (x < 1) x = 1;
  return dim3(static_cast<unsigned>(x), static_cast<unsigned>(y));
}

}  // namespace seld
