// Rational sample-rate conversion in front of the 24 kHz feature kernels (no upstream counterpart:
// the reference hands the file's rate to MelSpectrogram, dataset.py:27-58).
//
// Windowed-sinc polyphase FIR, zero delay, zero extension:  y[m] = sum_t x[q - (t - half)] * table[p][t],
// p = (m * down) mod up, q = (m * down) div up.  The table is the caller's ([up][taps] fp32 on the device;
// seld_resample_table_host evaluates the design of section 16.1 in double), so the kernel is a plain FIR with no state.
//
// Work split.  Outputs m = up * k + phi share the phase of phi, and their inputs are `down` samples apart.  A workgroup
// takes KT values of k for ALL up phases (a contiguous run of up * KT outputs); one wavefront works on one phase at a
// time, lane l on k = l (+ 64 r for R outputs per lane).  Consequences:
//   - the coefficient of a tap is the same for the whole wavefront: it is fetched by a scalar load from the table (L2 /
//     scalar cache resident, 80 - 173 KB for the 44.1 kHz family) and costs no vector or LDS slot;
//   - the input tile is staged once in LDS as fp32 (int16 scaled by 2^-15 on the way).  The 64 lanes of a tap read words
//     `down` apart: conflict-free as they lie when `down` is odd (147 for the 44.1 kHz family, 1 when up-sampling); for
//     an even `down` (2, 4, 8 for 48 / 96 / 192 kHz: 2-, 4-, 8-way conflicts) the tile is DE-INTERLEAVED by residue,
//     sample i at [i mod down][i div down], and the lanes read consecutive words of one row.  The taps are walked row
//     by row, so the address of a lane's next tap is always one word lower: no index arithmetic inside the loop;
//   - per tap and output: one ds_read_b32 and one v_fma_f32, the R accumulators of a lane are independent chains.
// All indices that can pass 2^31 (m, m * down, the sample index) are 64-bit; everything inside a tile is 32-bit.
#include <math.h>
#include <stdint.h>

#include <numeric>
#include <string>

#include "seld_common.h"

namespace seld {

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsMaxUp = 320;            // limits of the DESIGNED tables (seld_resample_plan); the kernel takes any table
constexpr int kRsMaxTaps = 1100;
constexpr int kRsZeroCrossings = 64;     // per side
constexpr double kRsBeta = 10.06;        // Kaiser
constexpr int kRsLdsFloats = 12288;      // preferred tile: 48 KB, three workgroups per CU
constexpr int kRsLdsFloatsMax = 16384;   // 64 KB: the dynamic LDS a launch gets without a function attribute

struct RsGeom {
  int up, down, taps, half;
  int kt;        // values of k per workgroup
  int chunks;    // ceil(kt / (64 R)): passes of one phase
  int pitch;     // words per residue row in LDS
  int tiles;     // workgroups per (clip, channel) row
  int rows;      // residue rows of the tile: down when down is even, else 1 (the samples as they lie)
  int stride;    // words between the samples of neighbouring lanes: down / rows
};

template <typename T>
__device__ __forceinline__ float rs_sample(const T* p);
template <>
__device__ __forceinline__ float rs_sample<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float rs_sample<int16_t>(const int16_t* p) { return static_cast<float>(*p) * (1.0f / 32768.0f); }

template <typename T, int R, bool kPlain>       // kPlain: rows == 1, the coefficients of consecutive taps are consecutive words
__global__ __launch_bounds__(kRsThreads) void resample_kernel(const T* __restrict__ pcm, const float* __restrict__ table,
                                                              float* __restrict__ out, long L, long L_out, RsGeom g) {
  extern __shared__ float rs_x[];                               // [rows][pitch]
  const int tid = threadIdx.x;
  const int row_id = blockIdx.x / g.tiles;                      // (clip, channel)
  const int tile = blockIdx.x - row_id * g.tiles;
  const long k0 = static_cast<long>(tile) * g.kt;
  const T* __restrict__ src = pcm + static_cast<long>(row_id) * L;
  float* __restrict__ dst = out + static_cast<long>(row_id) * L_out;

  // stage: tile sample i is x[k0 * down - half + i], zero outside [0, L)
  const long j0 = k0 * g.down - g.half;
  const int total = g.rows * g.pitch;
  for (int i = tid; i < total; i += kRsThreads) {
    const long j = j0 + i;
    float v = 0.0f;
    if (j >= 0 && j < L) v = rs_sample<T>(src + j);
    const int col = i / g.rows, row = i - col * g.rows;
    rs_x[row * g.pitch + col] = v;
  }
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int jobs = g.up * g.chunks;
  for (int job = wave; job < jobs; job += kRsWaves) {           // neighbouring phases run side by side: their stores
    const int chunk = job / g.up, phi = job - chunk * g.up;     // fill the same cache lines at about the same time
    const int pd = phi * g.down;                                // < 2^31: up <= 2^15, down <= 2^15 (checked by the host)
    const int qphi = pd / g.up, p = pd - qphi * g.up;
    const float* __restrict__ h = table + static_cast<long>(p) * g.taps;
    int kk[R], at[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      kk[r] = chunk * (64 * R) + lane + 64 * r;
      at[r] = (kk[r] < g.kt ? kk[r] : g.kt - 1) * g.stride;     // lanes past the tile read a valid word and store nothing
      acc[r] = 0.0f;
    }
    // tap t of output k reads tile sample k * down + u, u = qphi + 2 half - t >= 0: row u mod rows, column
    // k * stride + u div rows.  Row rho holds the taps t = first, first + rows, ...: u falls by rows, the column by one.
    const int u0 = qphi + 2 * g.half;
    const int rows = kPlain ? 1 : g.rows;
    for (int rho = 0; rho < rows; ++rho) {
      const int first = ((u0 - rho) % g.rows + g.rows) % g.rows;
      if (first >= g.taps) continue;
      const int count = (g.taps - first + g.rows - 1) / g.rows;
      const float* __restrict__ hp = h + first;
      const float* xw = rs_x + rho * g.pitch + (u0 - first - rho) / g.rows;
#pragma unroll 8
      for (int s = 0; s < count; ++s) {
        const float c = kPlain ? hp[s] : hp[static_cast<long>(s) * g.rows];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(xw[at[r] - s], c, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long m = (k0 + kk[r]) * g.up + phi;
      if (kk[r] < g.kt && m < L_out) dst[m] = acc[r];
    }
  }
}

// Tile geometry for (up, down, half): R outputs per lane and kt = 64 R x chunks values of k such that every wavefront has
// work and the de-interleaved tile fits; tables with a very large `down` fall back to fewer than 64 values of k.
static bool rs_geometry(int up, int down, int half, int* r_out, RsGeom* g) {
  g->rows = down % 2 == 0 ? down : 1;
  g->stride = down / g->rows;
  const int margin = 2 * half + down;                           // tile samples: kt * down + margin (u <= down - 1 + 2 half)
  auto fits = [&](long kt, int limit) {
    const long pitch = ((kt * down + margin + g->rows - 1) / g->rows) | 1;      // odd: the staging stores spread over the banks
    if (pitch * g->rows > limit) return false;
    g->kt = static_cast<int>(kt);
    g->pitch = static_cast<int>(pitch);
    return true;
  };
  const int want = (2 * kRsWaves + up - 1) / up;                // chunks for two jobs per wavefront
  for (int even = 1; even >= 0; --even)                         // first choice: the jobs divide evenly among the wavefronts
    for (int r : {4, 2, 1})
      for (int chunks = want; chunks >= 1; --chunks) {
        if ((even && (up * chunks) % kRsWaves != 0) || !fits(64L * r * chunks, kRsLdsFloats)) continue;
        *r_out = r;
        g->chunks = chunks;
        return true;
      }
  for (int kt = 64; kt >= 1; kt /= 2) {
    if (!fits(kt, kRsLdsFloatsMax)) continue;
    *r_out = 1;
    g->chunks = 1;
    return true;
  }
  return false;
}

template <typename T>
static int rs_launch(const char* name, const T* pcm, int64_t N, int64_t C, int64_t L, const float* table, int up, int down,
                     int taps, int half, float* out, int64_t L_out, void* stream_) {
  const std::string who(name);
  if (N < 0 || C < 0 || L < 0) return fail(kErrInvalidArgument, who + ": negative extent");
  if (up < 1 || down < 1 || up > 32768 || down > 32768 || half < 0 || half > 32768 || taps != 2 * half + 1)
    return fail(kErrInvalidArgument, who + ": needs 1 <= up, down <= 32768, 0 <= half <= 32768 and taps == 2 * half + 1");
  if (L > (INT64_MAX - down) / up) return fail(kErrInvalidArgument, who + ": L * up overflows");
  if (L_out != (L * up + down - 1) / down)
    return fail(kErrInvalidArgument, who + ": L_out must be ceil(L * up / down) = " + std::to_string((L * up + down - 1) / down));
  if (N == 0 || C == 0 || L_out == 0) return kOk;
  if (!pcm || !table || !out) return fail(kErrInvalidArgument, who + ": null pointer");
  RsGeom g{up, down, taps, half, 0, 0, 0, 0, 1, 1};
  int r = 1;
  if (!rs_geometry(up, down, half, &r, &g))
    return fail(kErrUnsupported, who + ": down = " + std::to_string(down) + " with " + std::to_string(taps) +
                                     " taps does not fit the 64 KB input tile");
  const long per_row = (L_out + up - 1) / up;                   // values of k
  const long tiles = (per_row + g.kt - 1) / g.kt;
  if (tiles * N * C > 0x7fffffffL || tiles > 0x7fffffffL) return fail(kErrUnsupported, who + ": more than 2^31 - 1 workgroups");
  g.tiles = static_cast<int>(tiles);
  const dim3 grid(static_cast<unsigned>(tiles * N * C)), block(kRsThreads);
  const size_t lds = static_cast<size_t>(g.rows) * g.pitch * sizeof(float);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const long Ll = L, Lo = L_out;
#define SELD_RS_LAUNCH(R_, PLAIN_) \
  hipLaunchKernelGGL((resample_kernel<T, R_, PLAIN_>), grid, block, lds, stream, pcm, table, out, Ll, Lo, g)
  if (g.rows == 1) {
    if (r == 4) SELD_RS_LAUNCH(4, true);
    else if (r == 2) SELD_RS_LAUNCH(2, true);
    else SELD_RS_LAUNCH(1, true);
  } else {
    if (r == 4) SELD_RS_LAUNCH(4, false);
    else if (r == 2) SELD_RS_LAUNCH(2, false);
    else SELD_RS_LAUNCH(1, false);
  }
#undef SELD_RS_LAUNCH
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

// ---- the design of DESIGN.md section 16.1, in double on the host ------------------------------------------------

struct RsPlan {
  int64_t rate_in, rate_out, fs, min_rate, n;
  int up, down, taps, half;
};

static int rs_plan(const char* who, int64_t rate_in, int64_t rate_out, RsPlan* plan) {
  if (rate_in <= 0 || rate_out <= 0 || rate_in > (1LL << 31) || rate_out > (1LL << 31))
    return fail(kErrInvalidArgument, std::string(who) + ": rates " + std::to_string(rate_in) + " -> " +
                                         std::to_string(rate_out) + " Hz: both must be positive (and below 2^31)");
  const int64_t gcd = std::gcd(rate_in, rate_out);
  const int64_t up = rate_out / gcd, down = rate_in / gcd;
  if (up > kRsMaxUp)
    return fail(kErrInvalidArgument, std::string(who) + ": rate " + std::to_string(rate_in) + " Hz -> " +
                                         std::to_string(rate_out) + " Hz needs up = " + std::to_string(up) +
                                         " phases, the limit is " + std::to_string(kRsMaxUp));
  plan->rate_in = rate_in;
  plan->rate_out = rate_out;
  plan->fs = rate_in * up;
  plan->min_rate = rate_in < rate_out ? rate_in : rate_out;
  // n = floor(T fs) with T fs = 64 fs / (0.95 min(r, R)) = 1280 fs / (19 min(r, R)): integers, no rounding question
  plan->n = (20 * kRsZeroCrossings * plan->fs) / (19 * plan->min_rate);
  const int64_t half = (plan->n + up - 1) / up, taps = 2 * half + 1;
  if (taps > kRsMaxTaps)
    return fail(kErrInvalidArgument, std::string(who) + ": rate " + std::to_string(rate_in) + " Hz -> " +
                                         std::to_string(rate_out) + " Hz needs " + std::to_string(taps) +
                                         " taps per output, the limit is " + std::to_string(kRsMaxTaps));
  plan->up = static_cast<int>(up);
  plan->down = static_cast<int>(down);
  plan->half = static_cast<int>(half);
  plan->taps = static_cast<int>(taps);
  return kOk;
}

// modified Bessel function I0 by its power series sum ((x/2)^k / k!)^2: all terms positive, converges for the beta used
static double rs_bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / (static_cast<double>(k) * static_cast<double>(k));
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

static double rs_prototype(const RsPlan& pl, int64_t i) {
  const int64_t a = i < 0 ? -i : i;
  if (a > pl.n) return 0.0;
  const double kPi = 3.14159265358979323846;
  const double tfs = static_cast<double>(20 * kRsZeroCrossings * pl.fs) / static_cast<double>(19 * pl.min_rate);
  const double cut = 0.95 * static_cast<double>(pl.min_rate) / static_cast<double>(pl.fs);      // 2 fc / fs
  const double ratio = static_cast<double>(a) / tfs;
  double w = 1.0 - ratio * ratio;
  if (w < 0.0) w = 0.0;
  const double window = rs_bessel_i0(kRsBeta * sqrt(w)) / rs_bessel_i0(kRsBeta);
  const double x = kPi * cut * static_cast<double>(a);
  const double sinc = a == 0 ? 1.0 : sin(x) / x;
  return static_cast<double>(pl.up) * cut * sinc * window;
}

}  // namespace seld

extern "C" {

int seld_resample_plan(int64_t rate_in, int64_t rate_out, int* up, int* down, int* taps, int* half) {
  using namespace seld;
  RsPlan pl;
  if (int rc = rs_plan("seld_resample_plan", rate_in, rate_out, &pl)) return rc;
  if (up) *up = pl.up;
  if (down) *down = pl.down;
  if (taps) *taps = pl.taps;
  if (half) *half = pl.half;
  return kOk;
}

int seld_resample_table_host(int64_t rate_in, int64_t rate_out, float* table, double* table_f64) {
  using namespace seld;
  RsPlan pl;
  if (int rc = rs_plan("seld_resample_table_host", rate_in, rate_out, &pl)) return rc;
  if (!table && !table_f64) return fail(kErrInvalidArgument, "seld_resample_table_host: both tables are null");
  for (int p = 0; p < pl.up; ++p)
    for (int t = 0; t < pl.taps; ++t) {
      const double v = rs_prototype(pl, p + static_cast<int64_t>(t - pl.half) * pl.up);
      const size_t at = static_cast<size_t>(p) * pl.taps + t;
      if (table_f64) table_f64[at] = v;
      if (table) table[at] = static_cast<float>(v);
    }
  return kOk;
}

int seld_resample_f32(const float* pcm, int64_t N, int64_t C, int64_t L, const float* table_dev, int up, int down, int taps,
                      int half, float* out, int64_t L_out, void* stream) {
  return seld::rs_launch<float>("seld_resample_f32", pcm, N, C, L, table_dev, up, down, taps, half, out, L_out, stream);
}

int seld_resample_i16(const int16_t* pcm, int64_t N, int64_t C, int64_t L, const float* table_dev, int up, int down, int taps,
                      int half, float* out, int64_t L_out, void* stream) {
  return seld::rs_launch<int16_t>("seld_resample_i16", pcm, N, C, L, table_dev, up, down, taps, half, out, L_out, stream);
}

}  // extern "C"
