// The one fp32 <-> bf16 conversion of libseld_hip.so's kernels, and the one typed accessor for V consecutive elements
// of a row.  Every kernel that stores bf16 rounds through pack_bf16x2 (v_cvt_pk_bf16_f32: round to nearest even, a NaN
// stays a NaN), so "the bf16 store rounding" the replay oracles model is one operation in the code as well.
// Device code only (hipcc); host-compiled cores such as logmel_core.h must not include it.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace seld {

// two floats -> one packed bf16 word (lo in bits 0..15): one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// one value, for scalar tails
__device__ __forceinline__ unsigned short bf16_bits(float v) {
  return static_cast<unsigned short>(pack_bf16x2(v, 0.0f));
}
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
// the value a bf16 store and reload leaves
__device__ __forceinline__ float round_bf16(float v) { return bf16_lo(pack_bf16x2(v, 0.0f)); }

// ---- V consecutive elements of a row as fp32, whatever the storage type; `elem` counts elements and is a multiple of V
// (bf16: one 16-byte access for V = 8, one 8-byte access for V = 4; fp32: V/4 16-byte accesses)
template <typename T, int V> struct Row;

template <int V> struct Row<__hip_bfloat16, V> {
  static_assert(V == 4 || V == 8, "8- or 16-byte accesses");
  static __device__ __forceinline__ void load(const void* base, long elem, float (&f)[V]) {
    const unsigned short* p = static_cast<const unsigned short*>(base) + elem;
    unsigned w[V / 2];
    if constexpr (V == 8) {
      const uint4 r = *reinterpret_cast<const uint4*>(p);
      w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
    } else {
      const uint2 r = *reinterpret_cast<const uint2*>(p);
      w[0] = r.x; w[1] = r.y;
    }
#pragma unroll
    for (int i = 0; i < V / 2; ++i) {
      f[2 * i] = bf16_lo(w[i]);
      f[2 * i + 1] = bf16_hi(w[i]);
    }
  }
  static __device__ __forceinline__ void store(void* base, long elem, const float (&f)[V]) {
    unsigned short* p = static_cast<unsigned short*>(base) + elem;
    unsigned w[V / 2];
#pragma unroll
    for (int i = 0; i < V / 2; ++i) w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    if constexpr (V == 8) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
  }
  static __device__ __forceinline__ float load1(const void* base, long elem) {
    return bf16_lo(static_cast<const unsigned short*>(base)[elem]);
  }
  static __device__ __forceinline__ float round(float v) { return round_bf16(v); }
};

template <int V> struct Row<float, V> {
  static_assert(V == 4 || V == 8, "16-byte accesses");
  static __device__ __forceinline__ void load(const void* base, long elem, float (&f)[V]) {
    const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(base) + elem);
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
      const float4 r = p[i];
      f[4 * i] = r.x; f[4 * i + 1] = r.y; f[4 * i + 2] = r.z; f[4 * i + 3] = r.w;
    }
  }
  static __device__ __forceinline__ void store(void* base, long elem, const float (&f)[V]) {
    float4* p = reinterpret_cast<float4*>(static_cast<float*>(base) + elem);
#pragma unroll
    for (int i = 0; i < V / 4; ++i) p[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
  }
  static __device__ __forceinline__ float load1(const void* base, long elem) {
    return static_cast<const float*>(base)[elem];
  }
  static __device__ __forceinline__ float round(float v) { return v; }
};

}  // namespace seld
