// Mixing two training windows inside the device window gather for gfx950, labels united.
//
// augment.hip moves a window's events (16 sign-and-swap transforms, SpecAugment masks); nothing there changes how many
// events a window holds.  Here window b, operand `a` (start starts[b], pattern of its parameter row), may get a PARTNER:
// another window of the same timeline with its own start sb, its own spatial pattern pb and a linear power gain g > 0
// (row b of `partners`, augment_core.h).  Per output frame w:
//   * row starts[b] + w outside the timeline: a zero row, features and labels;
//   * no partner, or row sb + w outside the timeline: the COPY path -- exactly what gather_augment_kernel /
//     permute_mask_kernel write, bit for bit (the value never goes through exp2 / log2);
//   * otherwise the MIX, defined on the stored features in the power domain (the powers of independent recordings add; the
//     per-bin cross term 2 Re(A conj B) is left out: the incoherent mix):
//       log-mel channel c:    power_to_db(P_a + g P_b),  P = 10^(x / 10) of the stored dB value x of the source channel the
//                             channel table names for the operand's pattern, P = 0 where x <= -100 (the floor);
//       intensity channel c:  (E_a IV_a + g E_b IV_b) / (E_a + g E_b), 0 where the denominator is 0, with
//                             E = P_W + (P_X + P_Y + P_Z) / 3 of the operand at that (frame, bin) and IV the SIGNED copy the
//                             channel table prescribes -- the band-level form of the normaliser the feature applies per bin;
//       label cell:           perm_pa(mask[starts[b] + w]) | perm_pb(mask[sb + w]).
//     Then the standardising map (kAffine), then the time / frequency masks of row `a` on the mixture; labels are never masked.
//
// Two feature kernels.  mix_chunks_kernel (no intensity channels) walks output chunks as gather_augment_kernel does: two
// 16-byte loads, one store.  mix_units_kernel (channels = 7: four log-mel + three intensity) walks UNITS as
// gather_rotate_kernel does: one thread produces the seven chunks of one (frame, 4-bin group) from fourteen loads, so E_a and
// E_b are formed once and the minimum is moved -- 2 x 7 chunks read, 7 written.  Channels are permuted by computed source
// address (signed_copy), never by indexing a register array with a runtime channel.
//
// All kernels: 16-byte stores only, no LDS, no scratch, no atomics; blockIdx.y walks the windows, so the parameter row, the
// partner row and both start frames are wave-uniform.  No value in `params` or `partners` can move a load or a store out of
// its array: patterns are reduced modulo 16, both starts only pass the row-in-timeline test, the gain is only multiplied.
#include "augment_core.h"

namespace seld {

constexpr float kLog2PerDb = 0.33219280948873623f;     // log2(10) / 10: P = 2^(x log2(10) / 10)
constexpr float kDbFloor = -100.0f;                    // power_to_db's floor: a stored value at or below it is power 0

// linear power of a stored dB value; one v_exp_f32, as power_to_db is one v_log_f32
__device__ __forceinline__ float db_to_power(float x) {
  return x > kDbFloor ? __builtin_amdgcn_exp2f(x * kLog2PerDb) : 0.0f;
}

struct Power4 {
  float x, y, z, w;
};

__device__ __forceinline__ Power4 chunk_power(uint4 v) {
  return {db_to_power(__uint_as_float(v.x)), db_to_power(__uint_as_float(v.y)), db_to_power(__uint_as_float(v.z)),
          db_to_power(__uint_as_float(v.w))};
}

// power_to_db(P_a + g P_b) on the four bins of a chunk: one fused multiply-add per bin
__device__ __forceinline__ uint4 mixed_db(const Power4& a, const Power4& b, float g) {
  return make_uint4(__float_as_uint(power_to_db(fmaf(g, b.x, a.x))), __float_as_uint(power_to_db(fmaf(g, b.y, a.y))),
                    __float_as_uint(power_to_db(fmaf(g, b.z, a.z))), __float_as_uint(power_to_db(fmaf(g, b.w, a.w))));
}

// (wa iva + wb ivb) r, r = 1 / (wa + wb) or 0: one bin of a mixed intensity channel
__device__ __forceinline__ unsigned mixed_iv(float wa, unsigned iva, float wb, unsigned ivb, float r) {
  return __float_as_uint(fmaf(wa, __uint_as_float(iva), __fmul_rn(wb, __uint_as_float(ivb))) * r);
}

// ---------------------------------------------------------------------------------------- features, per output chunk
// dst[b][w][c][f]: gather_augment_kernel's value, or the power mix with the partner's row.  Every channel is a log-mel channel.
template <bool kAffine>
__global__ void __launch_bounds__(256)
mix_chunks_kernel(const uint4* __restrict__ src, long total_rows, int channels, int freq_channels,
                  const int64_t* __restrict__ starts, const int32_t* __restrict__ params,
                  const int64_t* __restrict__ partners, long B, int window, const ChannelTable table, unsigned mask_bits,
                  const uint4* __restrict__ scale, const uint4* __restrict__ shift, uint4* __restrict__ dst) {
  const int row_chunks = channels * kChunksPerChannel;
  const int per_window = window * row_chunks;                       // host: < 2^31
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const Partner part = load_partner(partners, b);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    const unsigned long long packed_a = *reinterpret_cast<const unsigned long long*>(table.e[prm.pattern]);
    const unsigned long long packed_b = *reinterpret_cast<const unsigned long long*>(table.e[part.pattern]);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_chunks;
      const int chunk = q - w * row_chunks;
      const int c = chunk / kChunksPerChannel;
      const int fc = chunk - c * kChunksPerChannel;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        const unsigned entry_a = channels <= 8 ? packed_entry(packed_a, c) : table.e[prm.pattern][c];
        v = signed_copy(src + srow * row_chunks, entry_a, fc);
        const long brow = part.start + w;                           // wave-uniform, like srow
        if (part.on && brow >= 0 && brow < total_rows) {
          const unsigned entry_b = channels <= 8 ? packed_entry(packed_b, c) : table.e[part.pattern][c];
          const uint4 vb = signed_copy(src + brow * row_chunks, entry_b, fc);
          v = mixed_db(chunk_power(v), chunk_power(vb), part.gain);
        }
        v = standardised<kAffine>(v, scale, shift, chunk);
        v = masked(v, w, c, fc, prm, freq_channels, mask_bits);
      }
      to[q] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------- features, per unit (channels = 7)
constexpr int kMixMel = 4;                        // W X Y Z log-mel (in the recording's channel order)
constexpr int kMixIv = 3;                         // intensity channel 4 + n pairs W with input channel 1 + n
constexpr int kMixChannels = kMixMel + kMixIv;

// one output chunk of the unit through the standardising map and the masks of row `a`, to its place in the frame
template <bool kAffine>
__device__ __forceinline__ void store_unit_chunk(uint4 v, uint4* __restrict__ out, int w, int c, int fc,
                                                 const WindowParams& prm, int freq_channels, unsigned mask_bits,
                                                 const uint4* __restrict__ scale, const uint4* __restrict__ shift) {
  v = standardised<kAffine>(v, scale, shift, c * kChunksPerChannel + fc);
  out[c * kChunksPerChannel] = masked(v, w, c, fc, prm, freq_channels, mask_bits);
}

template <bool kAffine>
__global__ void __launch_bounds__(256)
mix_units_kernel(const uint4* __restrict__ src, long total_rows, int freq_channels, const int64_t* __restrict__ starts,
                 const int32_t* __restrict__ params, const int64_t* __restrict__ partners, long B, int window,
                 const ChannelTable8 table, unsigned mask_bits, const uint4* __restrict__ scale,
                 const uint4* __restrict__ shift, uint4* __restrict__ dst) {
  constexpr int row_chunks = kMixChannels * kChunksPerChannel;
  const int per_window = window * kChunksPerChannel;                // units; host: window * row_chunks < 2^31
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const WindowParams prm = load_params(params, b);
    const Partner part = load_partner(partners, b);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * (static_cast<long>(window) * row_chunks);
    const unsigned long long packed_a = *reinterpret_cast<const unsigned long long*>(table.e[prm.pattern]);
    const unsigned long long packed_b = *reinterpret_cast<const unsigned long long*>(table.e[part.pattern]);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / kChunksPerChannel;
      const int fc = q - w * kChunksPerChannel;
      const long srow = start + w;
      uint4* __restrict__ out = to + w * row_chunks + fc;
      if (!(srow >= 0 && srow < total_rows)) {
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int c = 0; c < kMixChannels; ++c) out[c * kChunksPerChannel] = zero;
        continue;
      }
      const uint4* __restrict__ row_a = src + srow * row_chunks;
      const long brow = part.start + w;                             // wave-uniform, like srow
      if (!(part.on && brow >= 0 && brow < total_rows)) {           // the copy path of gather_augment_kernel
#pragma unroll
        for (int c = 0; c < kMixChannels; ++c)
          store_unit_chunk<kAffine>(signed_copy(row_a, packed_entry(packed_a, c), fc), out, w, c, fc, prm, freq_channels,
                                    mask_bits, scale, shift);
        continue;
      }
      const uint4* __restrict__ row_b = src + brow * row_chunks;
      const float g = part.gain;
      Power4 ea, eb;                                                // E = P_W + (P_X + P_Y + P_Z) / 3, per bin
      Power4 sa{0.0f, 0.0f, 0.0f, 0.0f}, sb = sa;
#pragma unroll
      for (int c = 0; c < kMixMel; ++c) {
        const Power4 pa = chunk_power(signed_copy(row_a, packed_entry(packed_a, c), fc));
        const Power4 pb = chunk_power(signed_copy(row_b, packed_entry(packed_b, c), fc));
        store_unit_chunk<kAffine>(mixed_db(pa, pb, g), out, w, c, fc, prm, freq_channels, mask_bits, scale, shift);
        if (c == 0) {
          ea = pa;
          eb = pb;
        } else {
          sa.x += pa.x; sa.y += pa.y; sa.z += pa.z; sa.w += pa.w;
          sb.x += pb.x; sb.y += pb.y; sb.z += pb.z; sb.w += pb.w;
        }
      }
      constexpr float third = 1.0f / 3.0f;
      ea.x = fmaf(sa.x, third, ea.x); ea.y = fmaf(sa.y, third, ea.y); ea.z = fmaf(sa.z, third, ea.z); ea.w = fmaf(sa.w, third, ea.w);
      eb.x = g * fmaf(sb.x, third, eb.x); eb.y = g * fmaf(sb.y, third, eb.y);      // the partner's weight g E_b
      eb.z = g * fmaf(sb.z, third, eb.z); eb.w = g * fmaf(sb.w, third, eb.w);
      Power4 r;                                                     // 1 / (E_a + g E_b), 0 where both are silent
      r.x = ea.x + eb.x > 0.0f ? 1.0f / (ea.x + eb.x) : 0.0f;
      r.y = ea.y + eb.y > 0.0f ? 1.0f / (ea.y + eb.y) : 0.0f;
      r.z = ea.z + eb.z > 0.0f ? 1.0f / (ea.z + eb.z) : 0.0f;
      r.w = ea.w + eb.w > 0.0f ? 1.0f / (ea.w + eb.w) : 0.0f;
#pragma unroll
      for (int c = kMixMel; c < kMixChannels; ++c) {
        const uint4 ia = signed_copy(row_a, packed_entry(packed_a, c), fc);
        const uint4 ib = signed_copy(row_b, packed_entry(packed_b, c), fc);
        const uint4 v = make_uint4(mixed_iv(ea.x, ia.x, eb.x, ib.x, r.x), mixed_iv(ea.y, ia.y, eb.y, ib.y, r.y),
                                   mixed_iv(ea.z, ia.z, eb.z, ib.z, r.z), mixed_iv(ea.w, ia.w, eb.w, ib.w, r.w));
        store_unit_chunk<kAffine>(v, out, w, c, fc, prm, freq_channels, mask_bits, scale, shift);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- labels
// 8 consecutive destination cells of one operand: permute_mask_kernel's value (augment.hip) -- the 16-byte load for the
// identity, 2-byte source cells for every other pattern
__device__ __forceinline__ uint4 permuted_cells(const uint16_t* __restrict__ row, int chunk, int I, int J, int p) {
  if (p == 0) return reinterpret_cast<const uint4*>(row)[chunk];
  const bool mirror = (p >> 3) != 0, flip = (p & 1) != 0;
  const int shift = ((p >> 1) & 3) * (J / 4);
  int i2 = (chunk * 8) / J;                                         // destination cell (i2, j2)
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
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

// dst[b][w] = perm_pa(src[starts[b] + w]) | perm_pb(src[sb + w]); without a partner row: permute_mask_kernel's value
__global__ void __launch_bounds__(256)
mix_mask_kernel(const uint16_t* __restrict__ src, long total_rows, int I, int J, const int64_t* __restrict__ starts,
                const int32_t* __restrict__ params, const int64_t* __restrict__ partners, long B, int window,
                uint4* __restrict__ dst) {
  const int cells = I * J;
  const int row_chunks = cells / 8;
  const int per_window = window * row_chunks;                       // host: < 2^31
  for (long b = blockIdx.y; b < B; b += gridDim.y) {
    const int pa = params[b * kParamInts] & (kPatterns - 1);
    const Partner part = load_partner(partners, b);
    const long start = starts[b];
    uint4* __restrict__ to = dst + b * static_cast<long>(per_window);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per_window; q += gridDim.x * blockDim.x) {
      const int w = q / row_chunks;
      const int chunk = q - w * row_chunks;
      const long srow = start + w;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (srow >= 0 && srow < total_rows) {
        v = permuted_cells(src + srow * cells, chunk, I, J, pa);
        const long brow = part.start + w;
        if (part.on && brow >= 0 && brow < total_rows) {
          const uint4 vb = permuted_cells(src + brow * cells, chunk, I, J, part.pattern);
          v.x |= vb.x; v.y |= vb.y; v.z |= vb.z; v.w |= vb.w;
        }
      }
      to[q] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------- entry points
template <bool kAffine>
static int gather_mix(const char* who, const float* src, int64_t total_rows, int channels, int freq_channels,
                      const int64_t* starts, const int32_t* params, const int64_t* partners, int64_t B, int64_t window,
                      const uint8_t* channel_table, float mask_value, int iv_channels, const float* scale, const float* shift,
                      float* dst, void* stream_) {
  DeviceState* st;
  const int64_t row_chunks = static_cast<int64_t>(channels) * kChunksPerChannel;
  const bool extents_ok = channels > 0 && freq_channels >= 0 && freq_channels <= channels;
  const Refusal own[2] = {
      {channels > kMaxChannels, kErrUnsupported, "more than SELD_AUGMENT_MAX_CHANNELS feature channels"},
      {iv_channels != 0 && !(iv_channels == kMixIv && channels == kMixChannels), kErrUnsupported,
       "iv_channels must be 0 (every channel is log-mel) or 3 with 7 channels (log-mel + intensity vectors)"}};
  const int rc = kAffine ? check_window_args(who, total_rows, B, window, extents_ok, {own[0], own[1]}, row_chunks,
                                             {src, starts, params, partners, scale, shift, dst}, &st)
                         : check_window_args(who, total_rows, B, window, extents_ok, {own[0], own[1]}, row_chunks,
                                             {src, starts, params, partners, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (iv_channels == 0) {
    ChannelTable table;
    if (const int bad = fill_channel_table(who, channel_table, channels, &table)) return bad;
    hipLaunchKernelGGL(mix_chunks_kernel<kAffine>, window_grid(window * row_chunks, B, st->num_cus), dim3(256), 0, stream,
                       reinterpret_cast<const uint4*>(src), static_cast<long>(total_rows), channels, freq_channels, starts,
                       params, partners, static_cast<long>(B), static_cast<int>(window), table, mask_bits(mask_value),
                       reinterpret_cast<const uint4*>(scale), reinterpret_cast<const uint4*>(shift),
                       reinterpret_cast<uint4*>(dst));
  } else {
    ChannelTable8 table;
    if (const int bad = fill_channel_table(who, channel_table, channels, &table)) return bad;
    hipLaunchKernelGGL(mix_units_kernel<kAffine>, window_grid(window * kChunksPerChannel, B, st->num_cus), dim3(256), 0,
                       stream, reinterpret_cast<const uint4*>(src), static_cast<long>(total_rows), freq_channels, starts,
                       params, partners, static_cast<long>(B), static_cast<int>(window), table, mask_bits(mask_value),
                       reinterpret_cast<const uint4*>(scale), reinterpret_cast<const uint4*>(shift),
                       reinterpret_cast<uint4*>(dst));
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // namespace seld

extern "C" {

int seld_window_gather_mix(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                           const int32_t* params, const int64_t* partners, int64_t B, int64_t window,
                           const uint8_t* channel_table, float mask_value, int iv_channels, float* dst, void* stream_) {
  return seld::gather_mix<false>("seld_window_gather_mix", src, total_rows, channels, freq_channels, starts, params, partners,
                                 B, window, channel_table, mask_value, iv_channels, nullptr, nullptr, dst, stream_);
}

int seld_window_gather_mix_standardised(const float* src, int64_t total_rows, int channels, int freq_channels, const int64_t* starts,
                                  const int32_t* params, const int64_t* partners, int64_t B, int64_t window,
                                  const uint8_t* channel_table, float mask_value, int iv_channels, const float* scale,
                                  const float* shift, float* dst, void* stream_) {
  return seld::gather_mix<true>("seld_window_gather_mix_standardised", src, total_rows, channels, freq_channels, starts, params,
                                partners, B, window, channel_table, mask_value, iv_channels, scale, shift, dst, stream_);
}

int seld_window_mix_mask(const uint16_t* src, int64_t total_rows, int I, int J, const int64_t* starts, const int32_t* params,
                         const int64_t* partners, int64_t B, int64_t window, uint16_t* dst, void* stream_) {
  using namespace seld;
  const char* who = "seld_window_mix_mask";
  const int64_t cells = static_cast<int64_t>(I) * J;
  DeviceState* st;
  const int rc = check_window_args(
      who, total_rows, B, window, I > 0 && J > 0 && cells <= 65536,
      {{J % 4 != 0, kErrUnsupported, "a quarter turn is a whole number of cells only when J % 4 == 0"},
       {cells % 8 != 0, kErrUnsupported, "I*J must be a multiple of 8 (16-byte rows)"}},
      cells / 8, {src, starts, params, partners, dst}, &st);
  if (rc != kOk || B == 0) return rc;
  hipLaunchKernelGGL(mix_mask_kernel, window_grid(window * (cells / 8), B, st->num_cus), dim3(256), 0,
                     static_cast<hipStream_t>(stream_), src, static_cast<long>(total_rows), I, J, starts, params, partners,
                     static_cast<long>(B), static_cast<int>(window), reinterpret_cast<uint4*>(dst));
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
