// FOA rotation augmentation in azimuth steps of one grid cell (10 degrees on the 18 x 36 grid) inside the device window
// gather for gfx950.
//
// augment.hip gives a window one of the 16 sign-and-swap transforms: mirror m, k quarter turns, elevation flip e.  Here slot
// [9] of the same parameter row is an azimuth step r, and the window's transform is
//     mirror m,  then  s = (k J/4 + r) mod J  cells of azimuth  (phi = 2 pi s / J),  then  elevation flip e.
// The labels stay an exact cell permutation (a cyclic shift of the azimuth index by s): permute_mask_kernel<true> of
// augment.hip, behind seld_window_permute_mask_rotate.  The features do not stay a channel permutation: with c = cos phi,
// sn = sin phi and sigma = -1 after a mirror (else +1)
//     X' = c X - sn sigma Y,    Y' = sn X + c sigma Y,
// and log-mel(X') is no function of the stored log-mel channels.  The mel filterbank acts on POWERS, so three more mel rows
// per frame of the timeline -- P_X = mel |X|^2, P_Y = mel |Y|^2, C = mel Re(X conj Y), linear fp32, written once per
// recording by rotation_terms_kernel -- are all that is missing:
//     mel |X'|^2 = c^2 P_X + sn^2 P_Y - 2 c sn sigma C,      mel |Y'|^2 = sn^2 P_X + c^2 P_Y + 2 c sn sigma C.
// The intensity vectors are linear in the channels and their normaliser |W|^2 + (|X|^2 + |Y|^2 + |Z|^2) / 3 is rotation
// invariant:  IV_x' = c IV_x - sn sigma IV_y,  IV_y' = sn IV_x + c sigma IV_y.
//
// A window whose total s is a whole number of quarter turns takes the COPY path: the signed channel permutation of
// augment.hip under pattern (m, 4 s / J, e), bit for bit.  Every other window takes the rotated path.  The pair (cos, sin)
// comes from a [J][2] table the host builds in double precision and passes by value; it is wave-uniform (scalar loads), and
// no device sine or cosine is evaluated.
//
// gather_rotate_kernel walks UNITS, not output chunks: a unit is 16 bytes of one channel row, or -- for the X / Y log-mel
// pair and the IV_x / IV_y pair -- the same 16 bytes of BOTH outputs, produced by one thread from one set of loads (three
// rotation-term chunks, or the two intensity chunks).  Per frame at C = 4 that is 1280 B read + 1024 B written = 2304 B on
// the rotated path against the plain gather's 2048 B.  Every store is 16 bytes; no LDS, no scratch, no atomics.  As in
// augment.hip a parameter row is trusted no further than its bits: the pattern is reduced modulo 16, the step to 0..J-1 by
// a non-negative modulo, the masks are only compared with coordinates the kernel generates -- a row chooses WHICH in-bounds
// rows of the tables and the timeline are read, never an address outside them.
#include "augment_core.h"

namespace seld {

constexpr int kMaxSteps = SELD_ROTATE_MAX_STEPS;
constexpr int kRotTerms = 3;                          // P_X, P_Y, C
constexpr int kRotRowChunks = kRotTerms * kChunksPerChannel;
constexpr unsigned kNoChannel = 0xffu;

// ---------------------------------------------------------------------------------------- rotation terms (construction)
// One wavefront per frame, the structure of foa_iv_kernel (spatial.hip): the three per-bin products go to LDS rows, then
// the library's sparse mel pass -- lane j owns the <= 24 contiguous bins of filter j, mel[j] = A_j + B_{j-1}.
constexpr int kRtPitch = 512;                         // floats per product row in LDS (481 used, rest zero)
constexpr int kRtLdsFloatsPerWave = kRotTerms * kRtPitch + kRotTerms * 64;
constexpr int kRtWaves = 4;

struct RotTermArgs {
  const float* spec;     // [N][4][F][481] complex64
  float* out;
  long N, F;
  int ch_x, ch_y;
  long sN, sC, sM, sT;   // output strides (elements) of (clip, term 0..2, mel band, frame)
  LogmelTables tab;
};

__global__ __launch_bounds__(kRtWaves * 64) void rotation_terms_kernel(RotTermArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* rows = smem + wave * kRtLdsFloatsPerWave;           // [3][kRtPitch]
  float* bs = rows + kRotTerms * kRtPitch;                   // [3][64]
  for (int i = lane; i < kRotTerms * kRtPitch; i += 64) rows[i] = 0.0f;
  const int b0 = a.tab.mel_b0[lane];
  float wd[kMelMaxCnt], wu[kMelMaxCnt];
#pragma unroll
  for (int i = 0; i < kMelMaxCnt; ++i) {
    wd[i] = a.tab.mel_wd[i * 64 + lane];
    wu[i] = a.tab.mel_wu[i * 64 + lane];
  }
  const long frames_total = a.N * a.F;
  const long ch_stride = a.F * kBins;                        // complex elements between channels
  for (long f = static_cast<long>(blockIdx.x) * kRtWaves + wave; f < frames_total;
       f += static_cast<long>(gridDim.x) * kRtWaves) {
    const long n = f / a.F;
    const long t = f - n * a.F;
    const float2* base = reinterpret_cast<const float2*>(a.spec) + (n * 4 * a.F + t) * kBins;
    const float2* x_row = base + a.ch_x * ch_stride;
    const float2* y_row = base + a.ch_y * ch_stride;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = lane + 64 * r;
      if (k < kBins) {
        const float2 x = x_row[k], y = y_row[k];
        rows[k] = x.x * x.x + x.y * x.y;
        rows[kRtPitch + k] = y.x * y.x + y.y * y.y;
        rows[2 * kRtPitch + k] = x.x * y.x + x.y * y.y;      // Re(X conj Y)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float acc_a[kRotTerms];
#pragma unroll
    for (int c = 0; c < kRotTerms; ++c) {
      const float* p = rows + c * kRtPitch + b0;
      float sa = 0.0f, sb = 0.0f;
#pragma unroll
      for (int i = 0; i < kMelMaxCnt; ++i) {
        const float v = p[i];
        sa = fmaf(wd[i], v, sa);
        sb = fmaf(wu[i], v, sb);
      }
      acc_a[c] = sa;
      bs[c * 64 + lane] = sb;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float* outp = a.out + n * a.sN + lane * a.sM + t * a.sT;
#pragma unroll
    for (int c = 0; c < kRotTerms; ++c) {
      const float below = lane > 0 ? bs[c * 64 + lane - 1] : 0.0f;
      outp[c * a.sC] = acc_a[c] + below;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------------------- the rotating gathers
// Both travel BY VALUE (kernel argument memory), as the channel table (ChannelTable8 of augment_core.h) does.
struct RotationTable {                                // (cos, sin) of 2 pi s / J
  float cs[kMaxSteps][2];
};
struct UnitTable {                                    // byte n: the output channel(s) of unit slot n; second = 0xff: one only
  unsigned long long first, second;
  int slots;
};

// power_to_db(a P_X + b P_Y + g): g is the rounded cross term; four roundings on the longest chain (coefficient, cross
// product, two fused multiply-adds)
__device__ __forceinline__ unsigned rotated_db(float a, float px, float b, float py, float g) {
  return __float_as_uint(power_to_db(fmaf(a, px, fmaf(b, py, g))));
}

// kAffine (seld_window_gather_rotate_affine): every output chunk goes through scale / shift [channels][64] of ITS output
// channel before the masks (augment_core.h, standardised); the other instantiation never looks at the two pointers.
template <bool kAffine>
__global__ void __launch_bounds__(256)
gather_rotate_kernel(const uint4* __restrict__ src, const uint4* __restrict__ rot, long total_rows, int channels,
                     int freq_channels, int J, const int64_t* __restrict__ starts, const int32_t* __restrict__ params, long B,
                     int window, const ChannelTable8 table, const RotationTable angles, const UnitTable units,
                     unsigned mask_bits, const uint4* __restrict__ scale, const uint4* __restrict__ shift,
                     uint4* __restrict__ dst) {
  const int row_chunks = channels * kChunksPerChannel;
  const int row_units = units.slots * kChunksPerChannel;
  const int per_window = window * row_units;                        // host: < 2^31
  const int quarter = J / 4;
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const int m = prm.pattern >> 3, e = prm.pattern & 1;
    const int s = (((prm.pattern >> 1) & 3) * quarter + azimuth_step(params, b, J)) % J;
    const bool copy = s % quarter == 0;                             // a whole number of quarter turns: augment.hip's transform
    const int pattern = (m << 3) | (copy ? (s / quarter) << 1 : 0) | e;
    const unsigned long long packed = *reinterpret_cast<const unsigned long long*>(table.e[pattern]);
    const float c = angles.cs[s][0], sn = angles.cs[s][1];          // s < J <= kMaxSteps
    const float cg = m ? -c : c, sg = m ? -sn : sn;                 // times sigma
    const float c2 = __fmul_rn(c, c), s2 = __fmul_rn(sn, sn), x2 = 2.0f * __fmul_rn(c, sg);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * (static_cast<long>(window) * row_chunks);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_units;
      const int u = q - w * row_units;
      const int slot = u / kChunksPerChannel;
      const int fc = u - slot * kChunksPerChannel;
      const unsigned ca = static_cast<unsigned>(units.first >> (8 * slot)) & 0xffu;    // host: < channels
      const unsigned cb = static_cast<unsigned>(units.second >> (8 * slot)) & 0xffu;   // host: < channels, or kNoChannel
      const bool pair = cb != kNoChannel;
      const long srow = start + w;
      uint4 va = make_uint4(0u, 0u, 0u, 0u), vb = va;
      if (srow >= 0 && srow < total_rows) {
        const uint4* __restrict__ row = src + srow * row_chunks;
        if (copy || !pair) {
          va = signed_copy(row, packed_entry(packed, ca), fc);
          if (pair) vb = signed_copy(row, packed_entry(packed, cb), fc);
        } else if (ca < 4) {                                        // X' and Y' log-mel from the three rotation terms
          const uint4* __restrict__ terms = rot + srow * kRotRowChunks + fc;
          const uint4 px = terms[0], py = terms[kChunksPerChannel], cx = terms[2 * kChunksPerChannel];
          const float gx = __fmul_rn(x2, __uint_as_float(cx.x)), gy = __fmul_rn(x2, __uint_as_float(cx.y));
          const float gz = __fmul_rn(x2, __uint_as_float(cx.z)), gw = __fmul_rn(x2, __uint_as_float(cx.w));
          va = make_uint4(rotated_db(c2, __uint_as_float(px.x), s2, __uint_as_float(py.x), -gx),
                          rotated_db(c2, __uint_as_float(px.y), s2, __uint_as_float(py.y), -gy),
                          rotated_db(c2, __uint_as_float(px.z), s2, __uint_as_float(py.z), -gz),
                          rotated_db(c2, __uint_as_float(px.w), s2, __uint_as_float(py.w), -gw));
          vb = make_uint4(rotated_db(s2, __uint_as_float(px.x), c2, __uint_as_float(py.x), gx),
                          rotated_db(s2, __uint_as_float(px.y), c2, __uint_as_float(py.y), gy),
                          rotated_db(s2, __uint_as_float(px.z), c2, __uint_as_float(py.z), gz),
                          rotated_db(s2, __uint_as_float(px.w), c2, __uint_as_float(py.w), gw));
        } else {                                                    // IV_x' and IV_y' from the two stored vectors
          const uint4 ix = row[ca * kChunksPerChannel + fc], iy = row[cb * kChunksPerChannel + fc];
          const float x0 = __uint_as_float(ix.x), x1 = __uint_as_float(ix.y), x2v = __uint_as_float(ix.z), x3 = __uint_as_float(ix.w);
          const float y0 = __uint_as_float(iy.x), y1 = __uint_as_float(iy.y), y2 = __uint_as_float(iy.z), y3 = __uint_as_float(iy.w);
          va = make_uint4(__float_as_uint(fmaf(c, x0, -__fmul_rn(sg, y0))), __float_as_uint(fmaf(c, x1, -__fmul_rn(sg, y1))),
                          __float_as_uint(fmaf(c, x2v, -__fmul_rn(sg, y2))), __float_as_uint(fmaf(c, x3, -__fmul_rn(sg, y3))));
          vb = make_uint4(__float_as_uint(fmaf(sn, x0, __fmul_rn(cg, y0))), __float_as_uint(fmaf(sn, x1, __fmul_rn(cg, y1))),
                          __float_as_uint(fmaf(sn, x2v, __fmul_rn(cg, y2))), __float_as_uint(fmaf(sn, x3, __fmul_rn(cg, y3))));
        }
        va = standardised<kAffine>(va, scale, shift, static_cast<int>(ca) * kChunksPerChannel + fc);
        va = masked(va, w, static_cast<int>(ca), fc, prm, freq_channels, mask_bits);
        if (pair) {
          vb = standardised<kAffine>(vb, scale, shift, static_cast<int>(cb) * kChunksPerChannel + fc);
          vb = masked(vb, w, static_cast<int>(cb), fc, prm, freq_channels, mask_bits);
        }
      }
      uint4* __restrict__ out = to + w * row_chunks + fc;
      out[ca * kChunksPerChannel] = va;
      if (pair) out[cb * kChunksPerChannel] = vb;
    }
  }
}

// (cos, sin) of 2 pi s / J in double precision, rounded once; exactly 0 / +-1 at the quarter turns
static void fill_rotation_table(int J, RotationTable& t) {
  static const float kQuarter[4][2] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}, {0.0f, -1.0f}};
  for (int s = 0; s < kMaxSteps; ++s) {
    t.cs[s][0] = 1.0f;
    t.cs[s][1] = 0.0f;
    if (s >= J) continue;
    if ((4 * s) % J == 0) {
      t.cs[s][0] = kQuarter[4 * s / J][0];
      t.cs[s][1] = kQuarter[4 * s / J][1];
    } else {
      const double phi = 2.0 * M_PI * static_cast<double>(s) / static_cast<double>(J);
      t.cs[s][0] = static_cast<float>(cos(phi));
      t.cs[s][1] = static_cast<float>(sin(phi));
    }
  }
}

static bool is_xyz_permutation(int x, int y, int z) {
  return x >= 1 && x <= 3 && y >= 1 && y <= 3 && z >= 1 && z <= 3 && x != y && x != z && y != z;
}

// the two rotating feature entry points
template <bool kAffine>
static int gather_rotate(const char* who, const float* src, const float* rot, int64_t total_rows, int channels,
                         int freq_channels, int ch_x, int ch_y, int ch_z, int J, const int64_t* starts, const int32_t* params,
                         int64_t B, int64_t window, const uint8_t* channel_table, float mask_value, const float* scale,
                         const float* shift, float* dst, void* stream_) {
  DeviceState* st;
  const bool extents_ok = freq_channels >= 0 && freq_channels <= channels;
  const Refusal own[3] = {
      {channels != 4 && channels != 7, kErrUnsupported,
       "a rotation is defined for 4 (log-mel) or 7 (log-mel + intensity) FOA feature channels"},
      {!is_xyz_permutation(ch_x, ch_y, ch_z), kErrInvalidArgument, "ch_x, ch_y, ch_z must be a permutation of 1, 2, 3"},
      {J < 4 || J > kMaxSteps || J % 4 != 0, kErrUnsupported, "J must be a multiple of 4 in 4..SELD_ROTATE_MAX_STEPS"}};
  const int64_t frame_chunks = static_cast<int64_t>(channels) * kChunksPerChannel;
  const int rc = kAffine ? check_window_args(who, total_rows, B, window, extents_ok, {own[0], own[1], own[2]}, frame_chunks,
                                             {src, rot, starts, params, channel_table, scale, shift, dst}, &st)
                         : check_window_args(who, total_rows, B, window, extents_ok, {own[0], own[1], own[2]}, frame_chunks,
                                             {src, rot, starts, params, channel_table, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  ChannelTable8 table;
  if (const int bad = fill_channel_table(who, channel_table, channels, &table)) return bad;
  // unit slots in output-channel order; the Y channel rides in the X channel's slot
  UnitTable units{0ull, 0ull, 0};
  auto add = [&units](int a, int b) {
    units.first |= static_cast<unsigned long long>(a) << (8 * units.slots);
    units.second |= static_cast<unsigned long long>(b) << (8 * units.slots);
    ++units.slots;
  };
  for (int base = 0; base < channels - 1; base += 3)                // 0: W + log-mel X Y Z;  3: the intensity vectors
    for (int c = base == 0 ? 0 : 1; c <= 3; ++c) {
      if (c == ch_y) continue;
      if (c == ch_x) add(base + ch_x, base + ch_y);
      else add(base + c, static_cast<int>(kNoChannel));
    }
  RotationTable angles;
  fill_rotation_table(J, angles);
  const long per_window = window * units.slots * kChunksPerChannel;
  hipLaunchKernelGGL(gather_rotate_kernel<kAffine>, window_grid(per_window, B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), reinterpret_cast<const uint4*>(src),
                     reinterpret_cast<const uint4*>(rot), static_cast<long>(total_rows), channels, freq_channels, J, starts,
                     params, static_cast<long>(B), static_cast<int>(window), table, angles, units, mask_bits(mask_value),
                     reinterpret_cast<const uint4*>(scale), reinterpret_cast<const uint4*>(shift),
                     reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace seld

extern "C" {

int seld_foa_rotation_terms(const float* spec_complex, int64_t N, int64_t F, int ch_x, int ch_y, float* out, int64_t sN,
                            int64_t sC, int64_t sM, int64_t sT, void* stream_) {
  using namespace seld;
  DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!spec_complex || !out) return fail(kErrInvalidArgument, "seld_foa_rotation_terms: null pointer");
  if (N <= 0 || F <= 0) return fail(kErrInvalidArgument, "seld_foa_rotation_terms: N and F must be positive");
  if (ch_x < 1 || ch_x > 3 || ch_y < 1 || ch_y > 3 || ch_x == ch_y)
    return fail(kErrInvalidArgument, "seld_foa_rotation_terms: ch_x and ch_y must be two different channels of 1..3");
  RotTermArgs a{spec_complex, out, N, F, ch_x, ch_y, sN, sC, sM, sT, st->tables()};
  long blocks = (N * F + kRtWaves - 1) / kRtWaves;
  const long cap = static_cast<long>(st->num_cus) * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(rotation_terms_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kRtWaves * 64),
                     kRtWaves * kRtLdsFloatsPerWave * sizeof(float), static_cast<hipStream_t>(stream_), a);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_window_gather_rotate(const float* src, const float* rot, int64_t total_rows, int channels, int freq_channels,
                              int ch_x, int ch_y, int ch_z, int J, const int64_t* starts, const int32_t* params, int64_t B,
                              int64_t window, const uint8_t* channel_table, float mask_value, float* dst, void* stream_) {
  return seld::gather_rotate<false>("seld_window_gather_rotate", src, rot, total_rows, channels, freq_channels, ch_x, ch_y,
                                    ch_z, J, starts, params, B, window, channel_table, mask_value, nullptr, nullptr, dst,
                                    stream_);
}

int seld_window_gather_rotate_affine(const float* src, const float* rot, int64_t total_rows, int channels, int freq_channels,
                                     int ch_x, int ch_y, int ch_z, int J, const int64_t* starts, const int32_t* params,
                                     int64_t B, int64_t window, const uint8_t* channel_table, float mask_value,
                                     const float* scale, const float* shift, float* dst, void* stream_) {
  return seld::gather_rotate<true>("seld_window_gather_rotate_affine", src, rot, total_rows, channels, freq_channels, ch_x,
                                   ch_y, ch_z, J, starts, params, B, window, channel_table, mask_value, scale, shift, dst,
                                   stream_);
}

}  // extern "C"
