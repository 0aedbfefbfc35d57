// Global gradient norm of a LIST of tensors and the "guard" record the guarded Adam update reads (adam.hip,
// seld_multi_adam_guarded): clip coefficient, apply / skip decision, cumulative counters.  gfx950.
//
// One launch per 48 tensors plus one (two launches for up to 48 tensors, four for the ~150 of a model); deterministic (no atomics, no device-scope fences: the
// hand-off between the passes is the launch boundary).
//
//   pass 1  grad_sumsq_kernel   the work list of multi_adam_kernel (descriptors by value, no empty workgroups, one
//                               4096-element chunk per workgroup): reads the chunk of the gradient (bf16 or fp32, 16-byte
//                               loads when aligned, element-wise on ragged / unaligned tails), forms (g * grad_scale)^2 in
//                               fp32 and writes ONE fp32 partial per chunk with a plain vector store.
//   pass 2  guard_finish_kernel one workgroup: sums every partial in double in a fixed order, takes the root and writes
//                               the seld_guard_record.
//
// fp32 accumulation chain ahead of the double stage: 16 (per-thread serial, the first is an addition to 0) + 6 (wavefront,
// __shfl_down 32..1) + 3 (the four wavefront sums through LDS) = 25 additions of non-negative terms, <= 32: relative error
// of the sum <= 25 * 2^-24, of the root half that, plus one rounding of the result to fp32.
//
// A non-finite element makes its chunk's partial inf or NaN and with it the norm: no separate scan.  A FINITE gradient
// whose squares overflow fp32 within one chunk (elements above ~1e17 after grad_scale) also gives inf and counts as
// non-finite.
//
// Traffic: 2 B (bf16) or 4 B (fp32) per parameter read, 4 B per 4096 parameters written and read back: HBM-bound
// streaming, 4.7 M parameters of bf16 = 9.4 MB = 1.2 us at 8 TB/s (launch-latency bound in practice).
#include <hip/hip_bf16.h>

#include "seld_common.h"
#include "seld_hip.h"

namespace seld {

constexpr int kNormThreads = 256;
constexpr int kNormPerThread = 16;                       // 2 x 8 elements, the chunk of multi_adam_kernel
constexpr int kNormChunk = kNormThreads * kNormPerThread;
constexpr int kNormBatch = 48;

struct GradBatch {
  unsigned long long grad[kNormBatch];                   // bf16 or fp32 (flags bit 0: bf16)
  long n[kNormBatch];
  int first_block[kNormBatch];                           // work list: no empty workgroups
  int flags[kNormBatch];
  int count;
};

__global__ __launch_bounds__(kNormThreads) void grad_sumsq_kernel(const GradBatch b, const float grad_scale,
                                                                  float* __restrict__ partial) {
  __shared__ float wave_sum[kNormThreads / 64];
  int t = 0;
  while (t + 1 < b.count && static_cast<int>(blockIdx.x) >= b.first_block[t + 1]) ++t;      // uniform
  const long n = b.n[t];
  const long base = static_cast<long>(static_cast<int>(blockIdx.x) - b.first_block[t]) * kNormChunk;
  const bool grad_bf16 = b.flags[t] & 1;
  const unsigned short* gh = reinterpret_cast<const unsigned short*>(b.grad[t]);
  const float* gf = reinterpret_cast<const float*>(b.grad[t]);
  const bool aligned = (b.grad[t] & 15ull) == 0;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < kNormPerThread / 8; ++k) {
    const long i = base + (static_cast<long>(k) * kNormThreads + threadIdx.x) * 8;
    float g[8];
    if (aligned && i + 8 <= n) {
      if (grad_bf16) {
        const uint4 w = *reinterpret_cast<const uint4*>(gh + i);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          g[2 * j] = __uint_as_float(ww[j] << 16);
          g[2 * j + 1] = __uint_as_float(ww[j] & 0xffff0000u);
        }
      } else {
        const float4 a = *reinterpret_cast<const float4*>(gf + i), c = *reinterpret_cast<const float4*>(gf + i + 4);
        g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w; g[4] = c.x; g[5] = c.y; g[6] = c.z; g[7] = c.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long e = i + j;
        g[j] = e < n ? (grad_bf16 ? __uint_as_float(static_cast<unsigned>(gh[e]) << 16) : gf[e]) : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = g[j] * grad_scale;
      acc += s * s;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ __launch_bounds__(kNormThreads) void guard_finish_kernel(const float* __restrict__ partial, const long count,
                                                                    const float max_norm, const int skip_nonfinite,
                                                                    seld_guard_record* __restrict__ guard) {
  __shared__ double tree[kNormThreads];
  double acc = 0.0;
  for (long i = threadIdx.x; i < count; i += kNormThreads) acc += static_cast<double>(partial[i]);
  tree[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int width = kNormThreads / 2; width > 0; width >>= 1) {
    if (static_cast<int>(threadIdx.x) < width) tree[threadIdx.x] += tree[threadIdx.x + width];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = static_cast<float>(sqrt(tree[0]));
    float coef = 1.0f;
    if (max_norm > 0.0f) {
      const float q = max_norm / (norm + 1e-6f);         // torch.nn.utils.clip_grad_norm_
      coef = q > 1.0f ? 1.0f : q;                        // (a NaN norm stays a NaN coefficient, as torch's clamp keeps it)
    }
    const bool finite = fabsf(norm) <= 3.402823466e38f;  // false for inf and NaN
    const bool apply = finite || !skip_nonfinite;
    guard->grad_norm = norm;
    guard->clip_coef = coef;
    guard->apply = apply ? 1.0f : 0.0f;
    guard->skipped = apply ? 0.0f : 1.0f;
    guard->steps_skipped += apply ? 0 : 1;
    guard->steps_clipped += (apply && coef < 1.0f) ? 1 : 0;
  }
}

}  // namespace seld

extern "C" {

int seld_multi_grad_norm_scratch(const int64_t* lengths, int count, int64_t* partial_floats) {
  using namespace seld;
  if (count < 0 || (count > 0 && !lengths) || !partial_floats)
    return fail(kErrInvalidArgument, "seld_multi_grad_norm_scratch: bad arguments");
  int64_t chunks = 0;
  for (int i = 0; i < count; ++i) {
    if (lengths[i] <= 0) return fail(kErrInvalidArgument, "seld_multi_grad_norm_scratch: bad length");
    chunks += (lengths[i] + kNormChunk - 1) / kNormChunk;
  }
  *partial_floats = chunks > 0 ? chunks : 1;
  return kOk;
}

int seld_multi_grad_norm(const void* const* grad, const int32_t* grad_is_bf16, const int64_t* lengths, int count,
                         float grad_scale, float max_norm, int skip_nonfinite, float* partial, int64_t partial_floats,
                         seld_guard_record* guard, void* stream_) {
  using namespace seld;
  if (!current_state()) return kErrNotInitialised;
  if (count < 0) return fail(kErrInvalidArgument, "seld_multi_grad_norm: negative count");
  if (!partial || !guard || (count > 0 && (!grad || !grad_is_bf16 || !lengths)))
    return fail(kErrInvalidArgument, "seld_multi_grad_norm: null pointer");
  int64_t chunks = 0;
  for (int i = 0; i < count; ++i) {
    if (lengths[i] <= 0 || !grad[i]) return fail(kErrInvalidArgument, "seld_multi_grad_norm: bad tensor descriptor");
    chunks += (lengths[i] + kNormChunk - 1) / kNormChunk;
  }
  if (chunks > partial_floats) return fail(kErrInvalidArgument, "seld_multi_grad_norm: partial scratch too small");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  int64_t done = 0;                                       // chunks of the launches before this one
  for (int first = 0; first < count; first += kNormBatch) {
    GradBatch b;
    const int here = count - first < kNormBatch ? count - first : kNormBatch;
    long blocks = 0;
    for (int i = 0; i < here; ++i) {
      const int k = first + i;
      b.grad[i] = reinterpret_cast<unsigned long long>(grad[k]);
      b.n[i] = lengths[k];
      b.flags[i] = grad_is_bf16[k] ? 1 : 0;
      b.first_block[i] = static_cast<int>(blocks);
      blocks += (lengths[k] + kNormChunk - 1) / kNormChunk;
      if (blocks >= (1L << 31)) return fail(kErrUnsupported, "seld_multi_grad_norm: too many elements for one launch");
    }
    b.count = here;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kNormThreads), 0, stream, b, grad_scale,
                       partial + done);
    done += blocks;
  }
  hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(kNormThreads), 0, stream, partial, static_cast<long>(done), max_norm,
                     skip_nonfinite, guard);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
