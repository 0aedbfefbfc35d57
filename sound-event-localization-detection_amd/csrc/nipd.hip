// Mel-band NIPD (normalised inter-channel phase difference, the SALSA-Lite cue averaged over the mel bands; DESIGN.md
// section 23) from the Q15 phasor words of seld_logmel_phasors_* (logmel_core.h phase_c_store_phasors):
//
//   phi_m[k]  = atan2(Im, Re) of conj(P_0[k]) P_m[k] on the integers of the two words (exact in int32), 0 where either
//               word is 0 (a silent bin);                                  m = 1..C-1, channel 0 the reference
//   nipd_m[j] = sum_k W[k][j] phi_m[k],   W[k][j] = fb[k][j] (-c / (2 pi f_k)) / sum_{k' in range} fb[k'][j],   f_k = 25 k Hz
//
// for the bins in range (k >= 1, min_hz <= f_k <= max_hz): the extra acoustic path length to microphone m in metres, one
// value per mel band, 0 for a band without an in-range bin.  W is built on the host in double (seld_nipd_table_host) and
// handed to the kernel as a sparse table: first bin and tap count per band, at most 48 taps (the widest triangle of the
// filterbank, band 63, has 44 non-zero bins; the 24 of kMelMaxCnt counts only the bins a band OWNS in the log-mel kernel's
// two-weights-per-bin form).
//
// HBM-bound: a frame reads the in-range words of its C rows (79 of 481 at 50 - 2000 Hz: 8 x 336 B) and writes (C - 1) x
// 256 B.  One WAVEFRONT per frame, so the loop has no workgroup barrier: lane = (channel, four bins) while the phases are
// formed -- two 16-byte loads, four atan2f, one 16-byte LDS write -- then lane = mel band j, which walks its taps of every
// channel in ascending k with fmaf and writes the 64 floats of a channel row contiguously.  The band's weights stay in
// registers for the life of the wavefront.  No atomics, no scratch, no global workspace.
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "seld_common.h"
#include "logmel_tables.h"

namespace seld {

constexpr int kNipdMaxTaps = 48;                    // >= 44, the filterbank's widest band; a multiple of the tap groups of 8
constexpr int kNipdWaves = 4;
constexpr int kNipdTableInts = 2 * kMels;           // first_bin[64] | taps[64], then w[64][48] fp32
constexpr int kNipdTableBytes = kNipdTableInts * 4 + kMels * kNipdMaxTaps * 4;

struct NipdArgs {
  const uint32_t* phasors;     // [N][C][F][kPhasorPitch] words (re | im << 16)
  const int* table;            // first_bin[64] | taps[64] | w[64][48]
  float* out;                  // out[n*sN + (m-1)*sC + j + t*sT]
  unsigned total, F;           // frames of the call (N F < 2^31) and per clip
  int C;
  int u_lo, u_cnt;             // the 16-byte units (four bins) of a row that hold the table's bins: u_lo .. u_lo + u_cnt - 1
  long sN, sC, sT;
};

// atan2 of the exact integer product of two words; 0 when either is the silent word
__device__ __forceinline__ float nipd_phase(unsigned p0, unsigned pm) {
  const int re0 = static_cast<int>(p0 << 16) >> 16, im0 = static_cast<int>(p0) >> 16;
  const int rem = static_cast<int>(pm << 16) >> 16, imm = static_cast<int>(pm) >> 16;
  // |component| <= 32767, so both sums fit int32; formed modulo 2^32 because the words past bin 480 of a row, which share
  // the last 16-byte unit and are never read back, hold whatever the buffer held
  const int re = static_cast<int>(static_cast<unsigned>(re0) * static_cast<unsigned>(rem) +
                                  static_cast<unsigned>(im0) * static_cast<unsigned>(imm));
  const int im = static_cast<int>(static_cast<unsigned>(re0) * static_cast<unsigned>(imm) -
                                  static_cast<unsigned>(im0) * static_cast<unsigned>(rem));
  const float phi = atan2f(static_cast<float>(im), static_cast<float>(re));
  return (p0 == 0u || pm == 0u) ? 0.0f : phi;
}

__global__ __launch_bounds__(kNipdWaves * 64) void nipd_q15_kernel(NipdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int span = 4 * a.u_cnt;                                      // floats per channel row in LDS
  const int n_other = a.C - 1;
  float* ph = smem + wave * n_other * span;                          // [C - 1][span] phases of this wavefront's frame
  // lane j's band.  A table changed behind the library's check cannot read outside the rows: such a band is empty.
  const int k_first = 4 * a.u_lo;
  int first = a.table[lane], cnt = a.table[kMels + lane];
  if (cnt < 0 || cnt > kNipdMaxTaps || first < k_first || first + cnt > k_first + span) cnt = 0;
  const int base = cnt > 0 ? first - k_first : 0;
  const int last = cnt > 0 ? cnt - 1 : 0;
  float w[kNipdMaxTaps];
  const float* wt = reinterpret_cast<const float*>(a.table + kNipdTableInts) + lane * kNipdMaxTaps;
#pragma unroll
  for (int i = 0; i < kNipdMaxTaps; ++i) w[i] = i < cnt ? wt[i] : 0.0f;
  int cmax = cnt;                                                    // wavefront-uniform tap bound
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int other = __shfl_xor(cmax, off);
    cmax = other > cmax ? other : cmax;
  }
  cmax = __builtin_amdgcn_readfirstlane(cmax);
  const int items = n_other * span;                                  // (channel, bin) pairs of a frame
  const unsigned ch_stride = a.F * kPhasorPitch;                     // words between channel rows
  for (unsigned f = blockIdx.x * kNipdWaves + wave; f < a.total; f += gridDim.x * kNipdWaves) {
    const unsigned n = f / a.F, t = f - n * a.F;
    const uint32_t* row0 = a.phasors + (static_cast<unsigned long>(n) * a.C * a.F + t) * kPhasorPitch + k_first;
    for (int it = lane; it < items; it += 64) {
      const int m = it / span, k = it - m * span;
      ph[it] = nipd_phase(row0[k], row0[static_cast<unsigned>(m + 1) * ch_stride + k]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float* outp = a.out + n * a.sN + t * a.sT + lane;
    for (int m = 0; m < n_other; ++m) {
      const float* p = ph + m * span + base;
      float acc = 0.0f;
#pragma unroll
      for (int g = 0; g < kNipdMaxTaps / 8; ++g) {
        if (8 * g < cmax) {                                          // uniform: 9 taps at 50 - 2000 Hz walk 16, not 48
          // past the band's last tap the weight is 0 and the phase read again is the last tap's, a finite number: the
          // sum does not move (a lane mask per tap instead costs the loop two scalar registers per tap)
#pragma unroll
          for (int i = 8 * g; i < 8 * g + 8; ++i) acc = fmaf(w[i], p[i < last ? i : last], acc);
        }
      }
      outp[m * a.sC] = acc;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

struct NipdBand {
  int first = 0, taps = 0;
  double w[kNipdMaxTaps] = {};
};

// The table of one (range, speed), in double; an error text for a range this library refuses.
static const char* nipd_design(double min_hz, double max_hz, double speed, NipdBand (&bands)[kMels]) {
  if (!(min_hz >= 0.0) || !(max_hz <= 12000.0) || !(min_hz <= max_hz)) return "needs 0 <= min_hz <= max_hz <= 12000";
  if (!(speed > 0.0) || !std::isfinite(speed)) return "the speed of sound must be positive";
  std::vector<float> fb;
  default_mel_filterbank(fb);
  const double bin_hz = 12000.0 / (kBins - 1);                       // 25
  int in_range = 0;
  for (int k = 1; k < kBins; ++k) in_range += (k * bin_hz >= min_hz && k * bin_hz <= max_hz) ? 1 : 0;
  if (in_range == 0) return "no STFT bin lies in the range";
  for (int j = 0; j < kMels; ++j) {
    NipdBand& b = bands[j];
    b = NipdBand();
    double den = 0.0;
    int last = -1;
    for (int k = 1; k < kBins; ++k) {                                // ascending k
      const double v = fb[static_cast<size_t>(k) * kMels + j];
      if (v == 0.0 || k * bin_hz < min_hz || k * bin_hz > max_hz) continue;
      if (b.taps == 0) b.first = k;
      else if (k != last + 1) return "a mel band's bins are not contiguous";
      if (b.taps >= kNipdMaxTaps) return "a mel band holds more than 48 bins";
      b.w[b.taps++] = v;
      den += v;
      last = k;
    }
    for (int i = 0; i < b.taps; ++i)
      b.w[i] = b.w[i] * (-speed / (2.0 * M_PI * ((b.first + i) * bin_hz))) / den;
  }
  return nullptr;
}

// The table header as the library found it at `table` on its first use (a 512-byte read): its bins' span, or an error.
static int nipd_check_table(DeviceState* st, const void* table, hipStream_t stream, int* u_lo, int* u_cnt) {
  for (int i = 0; i < st->nipd_checked_n; ++i)
    if (st->nipd_checked[i].table == table) {
      *u_lo = st->nipd_checked[i].u_lo;
      *u_cnt = st->nipd_checked[i].u_cnt;
      return kOk;
    }
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  SELD_HIP_TRY(hipStreamIsCapturing(stream, &capturing));
  if (capturing != hipStreamCaptureStatusNone)
    return fail(kErrUnsupported, "seld_nipd_q15: a table's first use reads its header back; call once outside the capture");
  int header[kNipdTableInts];
  SELD_HIP_TRY(hipStreamSynchronize(stream));                        // an upload enqueued on the caller's stream
  SELD_HIP_TRY(hipMemcpy(header, table, sizeof(header), hipMemcpyDeviceToHost));
  int k_lo = kBins, k_hi = -1;
  for (int j = 0; j < kMels; ++j) {
    const int first = header[j], taps = header[kMels + j];
    if (taps < 0 || taps > kNipdMaxTaps)
      return fail(kErrInvalidArgument, "seld_nipd_q15: band " + std::to_string(j) + " of the table has " +
                                           std::to_string(taps) + " taps (0.." + std::to_string(kNipdMaxTaps) + ")");
    if (taps == 0) continue;
    if (first < 1 || first + taps > kBins)
      return fail(kErrInvalidArgument, "seld_nipd_q15: band " + std::to_string(j) + " of the table leaves bins 1..480");
    k_lo = first < k_lo ? first : k_lo;
    k_hi = first + taps - 1 > k_hi ? first + taps - 1 : k_hi;
  }
  if (k_hi < 0) return fail(kErrInvalidArgument, "seld_nipd_q15: the table has no taps");
  *u_lo = k_lo / 4;
  *u_cnt = k_hi / 4 - *u_lo + 1;
  constexpr int kSlots = sizeof(st->nipd_checked) / sizeof(st->nipd_checked[0]);
  const int slot = st->nipd_checked_n < kSlots ? st->nipd_checked_n++ : st->nipd_checked_next++ % kSlots;
  st->nipd_checked[slot] = {table, *u_lo, *u_cnt};
  return kOk;
}

}  // namespace seld

extern "C" {

int64_t seld_nipd_table_bytes(void) { return seld::kNipdTableBytes; }

int seld_nipd_table_host(double min_hz, double max_hz, double sound_speed, int32_t* first_bin, int32_t* taps, float* w,
                         double* w_f64) {
  using namespace seld;
  NipdBand bands[kMels];
  if (const char* why = nipd_design(min_hz, max_hz, sound_speed, bands))
    return fail(kErrInvalidArgument, std::string("seld_nipd_table_host: ") + why);
  for (int j = 0; j < kMels; ++j) {
    if (first_bin) first_bin[j] = bands[j].first;
    if (taps) taps[j] = bands[j].taps;
    for (int i = 0; i < kNipdMaxTaps; ++i) {
      if (w_f64) w_f64[j * kNipdMaxTaps + i] = bands[j].w[i];
      if (w) w[j * kNipdMaxTaps + i] = static_cast<float>(bands[j].w[i]);
    }
  }
  return kOk;
}

int seld_nipd_q15(const uint32_t* phasors, int64_t N, int64_t C, int64_t F, const void* table_dev, float* out, int64_t sN,
                  int64_t sC, int64_t sM, int64_t sT, void* stream_) {
  using namespace seld;
  DeviceState* st;
  if (int rc = check_pair_args("seld_nipd_q15", {phasors, table_dev, out}, N, C, F, kPhasorPitch, "phasors exceed 2^31 words", true, &st))
    return rc;
  if (!vector_rows(out, sN, sC, sM, sT))
    return fail(kErrUnsupported, "seld_nipd_q15: needs unit band stride and 16-byte aligned rows");
  if ((reinterpret_cast<uintptr_t>(phasors) & 15) != 0 || (reinterpret_cast<uintptr_t>(table_dev) & 3) != 0)
    return fail(kErrUnsupported, "seld_nipd_q15: phasor rows must be 16-byte aligned, the table 4-byte aligned");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int u_lo = 0, u_cnt = 0;
  if (int rc = nipd_check_table(st, table_dev, stream, &u_lo, &u_cnt)) return rc;
  NipdArgs a{phasors, static_cast<const int*>(table_dev), out, static_cast<unsigned>(N * F), static_cast<unsigned>(F),
             static_cast<int>(C), u_lo, u_cnt, sN, sC, sT};
  long blocks = (N * F + kNipdWaves - 1) / kNipdWaves;
  const long cap = static_cast<long>(st->num_cus) * 8;
  if (blocks > cap) blocks = cap;
  // (C - 1) x 4 u_cnt floats per wavefront: at most 4 x 7 x 484 x 4 = 54 208 B, inside the default dynamic-LDS limit
  const size_t lds = static_cast<size_t>(kNipdWaves) * (C - 1) * 4 * u_cnt * sizeof(float);
  hipLaunchKernelGGL(nipd_q15_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kNipdWaves * 64), lds, stream, a);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
