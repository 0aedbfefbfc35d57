// Multi-tensor Adam for the fp32-master / bf16-working-weight training mode (trainer.MasterWeightAdam), gfx950.
//
// The optimiser step of trainer.py:112-116, 179 upstream -- torch.optim.Adam(lr, weight_decay as L2 added to the gradient)
// -- ran here as THREE multi-tensor launches: bf16 gradients -> fp32 (seld_multi_cast), the framework's fused Adam on the
// fp32 masters, fp32 masters -> bf16 working copies (seld_multi_cast): 40 bytes of HBM traffic per parameter.  This
// kernel reads the bf16 gradient itself and writes the bf16 working copy itself: gradient 2 (or 4) + master 4 + exp_avg 4
// + exp_avg_sq 4 read, 4 + 4 + 4 (+ 2) written = 28 B per parameter, one launch per 48 tensors, descriptors by value
// (the seld_multi_cast pattern: gradient tensors that autograd re-allocates every iteration need no descriptor upload).
// Pure HBM-bound elementwise work.
//
// Arithmetic: the formulas of the framework's fused kernel (ATen fused_adam_utils.cuh, ADAM_MODE::ORIGINAL, amsgrad off,
// maximize off), in fp32:   g += weight_decay * p;   m = m + (1 - beta1) (g - m);   v = beta2 v + (1 - beta2) g g;
//            p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
// with lr and step read from DEVICE scalars (graph replay: a ReduceLROnPlateau change needs no re-capture; the caller
// increments step before the launch).  As there, the betas arrive as DOUBLES: 1 - beta and 1 - beta^step are formed in
// double and rounded once (1 - 0.999f is 1.3e-5 off 0.001, and that error went straight into v and into the step size
// while everything was float).  The element chain is fp32 with this file's own contractions, so the result agrees with
// the framework's to rounding, not bit for bit: tests/test_adam_edges_gpu.py holds the update's relative error against
// float64 Adam to twice the framework kernel's own.
//
// multi_adam_guarded_kernel is the same body with three additions (seld_multi_adam_guarded): it reads
// the guard record of csrc/guard.hip and returns before its first store when the step is skipped, multiplies the gradient
// by the clip coefficient after grad_scale (a coefficient of exactly 1 gives the plain kernel's bits), and keeps an fp32
// exponential moving average of the new masters in the same pass: + 8 B per parameter (ema read and written) on the 28 B.
#include "seld_bf16.h"
#include "seld_common.h"
#include "seld_hip.h"

namespace seld {

constexpr int kAdamThreads = 256;
constexpr int kAdamPerThread = 16;                       // 2 x 8 elements
constexpr int kAdamChunk = kAdamThreads * kAdamPerThread;
constexpr int kAdamBatch = 48;

struct AdamBatch {
  unsigned long long grad[kAdamBatch];                   // bf16 or fp32 (flags bit 0: bf16)
  unsigned long long param[kAdamBatch];                  // fp32 master / parameter
  unsigned long long m[kAdamBatch];                      // exp_avg, fp32
  unsigned long long v[kAdamBatch];                      // exp_avg_sq, fp32
  unsigned long long low[kAdamBatch];                    // bf16 working copy, or 0
  long n[kAdamBatch];
  int first_block[kAdamBatch];                           // work list: no empty workgroups
  int flags[kAdamBatch];
  int count;
};

struct AdamScalars {
  const float* lr;
  const float* step;
  double beta1, beta2;
  float eps, weight_decay, grad_scale;
};

// beta^step in double for the optimiser's whole-number step count (< 2^24: exact in the fp32 scalar), by squaring: at most
// 48 multiplications, wave-uniform.
__device__ __forceinline__ double adam_beta_power(double beta, float step) {
  unsigned n = static_cast<unsigned>(step);
  double r = 1.0;
  while (n) {
    if (n & 1u) r *= beta;
    beta *= beta;
    n >>= 1;
  }
  return r;
}

struct AdamGuard {
  unsigned long long ema[kAdamBatch];                    // fp32 moving average of the master, or 0
  const seld_guard_record* guard;                        // or nullptr: always apply, coefficient 1
  float ema_rate;                                        // 1 - decay
};

template <bool kGuarded>
__device__ __forceinline__ void multi_adam_body(const AdamBatch& b, const AdamScalars& s, const AdamGuard* x) {
  float coef = 1.0f;
  if (kGuarded && x->guard) {
    if (x->guard->apply == 0.0f) return;                 // uniform: the whole grid leaves before any store
    coef = x->guard->clip_coef;
  }
  int t = 0;
  while (t + 1 < b.count && static_cast<int>(blockIdx.x) >= b.first_block[t + 1]) ++t;      // uniform
  const long n = b.n[t];
  const long base = static_cast<long>(static_cast<int>(blockIdx.x) - b.first_block[t]) * kAdamChunk;
  const bool grad_bf16 = b.flags[t] & 1;
  const unsigned short* gh = reinterpret_cast<const unsigned short*>(b.grad[t]);
  const float* gf = reinterpret_cast<const float*>(b.grad[t]);
  float* p = reinterpret_cast<float*>(b.param[t]);
  float* m = reinterpret_cast<float*>(b.m[t]);
  float* v = reinterpret_cast<float*>(b.v[t]);
  unsigned short* low = reinterpret_cast<unsigned short*>(b.low[t]);
  float* ema = kGuarded ? reinterpret_cast<float*>(x->ema[t]) : nullptr;
  const float lr = *s.lr, step = *s.step;
  const float bc1 = static_cast<float>(1.0 - adam_beta_power(s.beta1, step));
  const float bc2 = static_cast<float>(1.0 - adam_beta_power(s.beta2, step));
  const float step_size = lr / bc1, bc2_sqrt = sqrtf(bc2);
  const float beta2 = static_cast<float>(s.beta2);
  const float rest1 = static_cast<float>(1.0 - s.beta1), rest2 = static_cast<float>(1.0 - s.beta2);
  const bool aligned = ((b.grad[t] | b.param[t] | b.m[t] | b.v[t] | b.low[t] | (kGuarded ? x->ema[t] : 0ull)) & 15ull) == 0;
#pragma unroll
  for (int k = 0; k < kAdamPerThread / 8; ++k) {
    const long i = base + (static_cast<long>(k) * kAdamThreads + threadIdx.x) * 8;
    if (i >= n) break;
    float g[8], pp[8], mm[8], vv[8], ee[8];
    const bool full = aligned && i + 8 <= n;
    if (full) {
      if (grad_bf16) Row<__hip_bfloat16, 8>::load(gh, i, g);
      else Row<float, 8>::load(gf, i, g);
      Row<float, 8>::load(p, i, pp);
      Row<float, 8>::load(m, i, mm);
      Row<float, 8>::load(v, i, vv);
      if (kGuarded && ema) Row<float, 8>::load(ema, i, ee);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const long e = i + j < n ? i + j : n - 1;
        g[j] = grad_bf16 ? bf16_lo(gh[e]) : gf[e];
        pp[j] = p[e];
        mm[j] = m[e];
        vv[j] = v[e];
        if (kGuarded && ema) ee[j] = ema[e];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gj = g[j] * s.grad_scale;
      if (kGuarded) gj *= coef;
      gj = fmaf(s.weight_decay, pp[j], gj);
      mm[j] = fmaf(rest1, gj - mm[j], mm[j]);
      vv[j] = fmaf(beta2, vv[j], rest2 * gj * gj);
      const float denom = sqrtf(vv[j]) / bc2_sqrt + s.eps;
      pp[j] -= step_size * mm[j] / denom;
      if (kGuarded && ema) ee[j] = fmaf(x->ema_rate, pp[j] - ee[j], ee[j]);
    }
    if (full) {
      Row<float, 8>::store(p, i, pp);
      Row<float, 8>::store(m, i, mm);
      Row<float, 8>::store(v, i, vv);
      if (low) Row<__hip_bfloat16, 8>::store(low, i, pp);
      if (kGuarded && ema) Row<float, 8>::store(ema, i, ee);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (i + j < n) {
          p[i + j] = pp[j];
          m[i + j] = mm[j];
          v[i + j] = vv[j];
          if (low) low[i + j] = bf16_bits(pp[j]);
          if (kGuarded && ema) ema[i + j] = ee[j];
        }
      }
    }
  }
}

__global__ __launch_bounds__(kAdamThreads) void multi_adam_kernel(const AdamBatch b, const AdamScalars s) {
  multi_adam_body<false>(b, s, nullptr);
}

__global__ __launch_bounds__(kAdamThreads) void multi_adam_guarded_kernel(const AdamBatch b, const AdamScalars s,
                                                                          const AdamGuard x) {
  multi_adam_body<true>(b, s, &x);
}

}  // namespace seld

extern "C" {

int seld_multi_adam(const void* const* grad, const int32_t* grad_is_bf16, float* const* param, float* const* exp_avg,
                    float* const* exp_avg_sq, void* const* low_bf16, const int64_t* lengths, int count, const float* lr,
                    const float* step, double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                    void* stream_) {
  using namespace seld;
  if (!current_state()) return kErrNotInitialised;
  if (count < 0) return fail(kErrInvalidArgument, "seld_multi_adam: negative count");
  if (count == 0) return kOk;
  if (!grad || !grad_is_bf16 || !param || !exp_avg || !exp_avg_sq || !low_bf16 || !lengths || !lr || !step)
    return fail(kErrInvalidArgument, "seld_multi_adam: null pointer");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const AdamScalars s{lr, step, beta1, beta2, eps, weight_decay, grad_scale};
  for (int first = 0; first < count; first += kAdamBatch) {
    AdamBatch b;
    const int here = count - first < kAdamBatch ? count - first : kAdamBatch;
    long blocks = 0;
    for (int i = 0; i < here; ++i) {
      const int k = first + i;
      if (lengths[k] <= 0 || !grad[k] || !param[k] || !exp_avg[k] || !exp_avg_sq[k])
        return fail(kErrInvalidArgument, "seld_multi_adam: bad tensor descriptor");
      b.grad[i] = reinterpret_cast<unsigned long long>(grad[k]);
      b.param[i] = reinterpret_cast<unsigned long long>(param[k]);
      b.m[i] = reinterpret_cast<unsigned long long>(exp_avg[k]);
      b.v[i] = reinterpret_cast<unsigned long long>(exp_avg_sq[k]);
      b.low[i] = reinterpret_cast<unsigned long long>(low_bf16[k]);
      b.n[i] = lengths[k];
      b.flags[i] = grad_is_bf16[k] ? 1 : 0;
      b.first_block[i] = static_cast<int>(blocks);
      blocks += (lengths[k] + kAdamChunk - 1) / kAdamChunk;
      if (blocks >= (1L << 31)) return fail(kErrUnsupported, "seld_multi_adam: too many elements for one launch");
    }
    b.count = here;
    hipLaunchKernelGGL(multi_adam_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kAdamThreads), 0, stream, b, s);
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_multi_adam_guarded(const void* const* grad, const int32_t* grad_is_bf16, float* const* param,
                            float* const* exp_avg, float* const* exp_avg_sq, void* const* low_bf16, const int64_t* lengths,
                            int count, const float* lr, const float* step, double beta1, double beta2, float eps,
                            float weight_decay, float grad_scale, float* const* ema, float ema_decay,
                            const seld_guard_record* guard, void* stream_) {
  using namespace seld;
  if (!current_state()) return kErrNotInitialised;
  if (count < 0) return fail(kErrInvalidArgument, "seld_multi_adam_guarded: negative count");
  if (count == 0) return kOk;
  if (!grad || !grad_is_bf16 || !param || !exp_avg || !exp_avg_sq || !low_bf16 || !lengths || !lr || !step)
    return fail(kErrInvalidArgument, "seld_multi_adam_guarded: null pointer");
  if (!(ema_decay >= 0.0f && ema_decay < 1.0f)) return fail(kErrInvalidArgument, "seld_multi_adam_guarded: ema_decay not in [0, 1)");
  const bool with_ema = ema != nullptr && ema_decay != 0.0f;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const AdamScalars s{lr, step, beta1, beta2, eps, weight_decay, grad_scale};
  for (int first = 0; first < count; first += kAdamBatch) {
    AdamBatch b;
    AdamGuard x;
    const int here = count - first < kAdamBatch ? count - first : kAdamBatch;
    long blocks = 0;
    for (int i = 0; i < here; ++i) {
      const int k = first + i;
      if (lengths[k] <= 0 || !grad[k] || !param[k] || !exp_avg[k] || !exp_avg_sq[k])
        return fail(kErrInvalidArgument, "seld_multi_adam_guarded: bad tensor descriptor");
      b.grad[i] = reinterpret_cast<unsigned long long>(grad[k]);
      b.param[i] = reinterpret_cast<unsigned long long>(param[k]);
      b.m[i] = reinterpret_cast<unsigned long long>(exp_avg[k]);
      b.v[i] = reinterpret_cast<unsigned long long>(exp_avg_sq[k]);
      b.low[i] = reinterpret_cast<unsigned long long>(low_bf16[k]);
      x.ema[i] = with_ema ? reinterpret_cast<unsigned long long>(ema[k]) : 0ull;
      b.n[i] = lengths[k];
      b.flags[i] = grad_is_bf16[k] ? 1 : 0;
      b.first_block[i] = static_cast<int>(blocks);
      blocks += (lengths[k] + kAdamChunk - 1) / kAdamChunk;
      if (blocks >= (1L << 31)) return fail(kErrUnsupported, "seld_multi_adam_guarded: too many elements for one launch");
    }
    b.count = here;
    x.guard = guard;
    x.ema_rate = 1.0f - ema_decay;
    hipLaunchKernelGGL(multi_adam_guarded_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kAdamThreads), 0, stream, b, s, x);
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
