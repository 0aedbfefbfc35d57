// First encoder block (model_crnn.py:5-17 ConvBlock with 4 -> 64 channels) on gfx950:
//
//   Conv3x3(4 -> 64, stride 1, pad 1, no bias) -> BatchNorm2d (training) -> ReLU -> MaxPool2d((1, 2))
//
// with the convolution RECOMPUTED inside every kernel that needs its output instead of stored.  The convolution is
// 36 MACs per output (2.4 GFLOP at batch 32: ~2 us of the chip's matrix time) while its bf16 output x1 is 65.5 MB and
// its gradient dx1 another 65.5 MB; the block's real operands are the 4 MB input, the 33 MB pooled output and the
// 33 MB pooled gradient.  Block 1 has no data gradient (its input is data), so dx1 only ever feeds the weight gradient.
//
//   forward  1  stats    : in -> conv -> sum / sum of squares (in double) partials per channel       (x1 not written)
//               finalise : partials -> mean / invstd / a, b, running statistics                      (8 small workgroups)
//            2  apply    : in -> conv -> max_pair(relu(round(a x + b))) -> y
//   backward 3  reduce   : in, dy -> conv -> routing (ReLU gate, first-wins argmax) -> sum dz, sum dz x partials
//               finalise : partials -> dgamma, dbeta, p, q
//            4  wgrad    : in, dy -> conv -> dx1 = a dz + p + q x rounded to bf16 -> dW1 partial = dx1^T * im2col(in)
//                          by MFMA                                                                    (dx1 not written)
//            5  sum      : fixed-order sum of the per-workgroup partials into dW1 (parameter's strides and dtype)
//
// The kernels are bound by the vector ALU (32.8 M convolution outputs: 0.8 us of the chip per instruction and value),
// not by HBM or the matrix cores, so everything that can be a matrix product is one: the rounded bf16 outputs leave the
// ALU packed in exactly the register layout of an MFMA operand over the wave's positions (cf_operand), and the channel
// sums, sums of squares, sum dz x and the weight gradient itself are products of such operands.
//
// All four big kernels call the same cf_conv_tile(): x1 = round_bf16(conv) with fp32 accumulation in one fixed order,
// so the ReLU mask and pooling argmax recomputed by the backward pass agree bit for bit with the forward's.  The
// expressions after the convolution are those of convtail.hip (tail_apply_kernel<bf16, 2>, route<bf16, 2>, the two
// finalise kernels).  No atomics, no fences: kernel boundaries publish the partials; same inputs, same bits.
//
// Geometry.  The input is channels-last, in[b][t][f][4]: a position's 4 channels are 8 bytes.  A workgroup (4 waves)
// takes chunks of 256 positions = 256 / F consecutive time rows of one clip and keeps the rows t0-1 .. t0+TC with a
// zero column on either frequency edge in LDS (rows outside [0, T) are zero).  The convolution of 16 consecutive
// positions (one time row, F % 16 == 0) is a 16 x 64 x 36 product, K padded to 64: two v_mfma_f32_16x16x32_bf16 per
// 16 channels.  A = positions x (tap, ci): lane (g, i) reads the 8 bytes of taps 2g and 2g+1 at position i straight
// from the image (no transpose needed); B = the weights, held in registers for the whole kernel.  B's column n of
// tile nt is channel 4 n + nt, so a lane ends up with FOUR ADJACENT CHANNELS (4 c .. 4 c + 3, c = lane & 15) of four
// adjacent positions (4 g .. 4 g + 3): both bins of a pooling pair are in the lane, a pooled output's 4 channels are
// one 8-byte access and 16 lanes cover a full 128-byte row of y / dy.
#include "seld_bf16.h"
#include "seld_common.h"

namespace seld {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kCfThreads = 256;
constexpr int kCfPos = 256;                 // positions per chunk
constexpr int kCfTiles = kCfPos / 16;       // 16-position tiles per chunk, 4 per wave
constexpr int kCfCout = 64;
constexpr int kCfCin = 4;
constexpr int kCfK = 36;                    // 9 taps x 4 input channels
constexpr int kCfMaxGroups = 512;           // workgroups = partial rows, at most
constexpr int kCfImage = 3 * 258;           // image positions, largest case (F = 256: 3 rows of 258)
constexpr int kCfStage = 3;                 // 8-byte pieces per thread per chunk, largest case
constexpr int kCfSumThreads = 256;
constexpr int kCfSumRows = 16;

struct CfGeom {
  int T, logF, chunks_per_clip, chunks;
  long rows;                                // B * T * F
};

struct CfWeights {                          // the convolution weight [64][4][3][3] with its strides (elements)
  const void* w;
  int is_bf16;
  int packed;                               // bf16, dense [64][3][3][4] (channels-last memory), 8-byte aligned
  long sco, sci, sr, ss;
};

__device__ __forceinline__ float cf_weight(const CfWeights& w, int co, int tap, int ci) {
  const long i = co * w.sco + ci * w.sci + (tap / 3) * w.sr + (tap % 3) * w.ss;
  if (w.is_bf16) return bf16_lo(static_cast<const unsigned short*>(w.w)[i]);
  return round_bf16(static_cast<const float*>(w.w)[i]);       // the cast autocast would do
}

// B fragments: wb[nt][ks], column n = lane & 15 is channel 4 n + nt, k = 8 g + e is (tap 2 g + e / 4, ci e % 4) of
// K step ks = 0 and tap 8 (g = 0, e < 4; zero otherwise) of K step 1
__device__ __forceinline__ void cf_load_weights(const CfWeights& w, int lane, bf16x8 (&wb)[4][2]) {
  const int g = lane >> 4, c = lane & 15;
  if (w.packed) {                           // a lane's 8 values of K step 0 are one 16-byte run, tap 8 one 8-byte run
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const uint2* const row = reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(w.w) + (4 * c + nt) * kCfK);
      const uint2 lo = row[2 * g], hi = row[2 * g + 1];
      uint2 last = row[8];
      if (g != 0) last = make_uint2(0u, 0u);
      const u32x4 p0 = {lo.x, lo.y, hi.x, hi.y}, p1 = {last.x, last.y, 0u, 0u};
      wb[nt][0] = __builtin_bit_cast(bf16x8, p0);
      wb[nt][1] = __builtin_bit_cast(bf16x8, p1);
    }
    return;
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int co = 4 * c + nt;
    float v0[8], v1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v0[e] = cf_weight(w, co, 2 * g + (e >> 2), e & 3);
      v1[e] = (g == 0 && e < 4) ? cf_weight(w, co, 8, e & 3) : 0.0f;
    }
    const u32x4 p0 = {pack_bf16x2(v0[0], v0[1]), pack_bf16x2(v0[2], v0[3]), pack_bf16x2(v0[4], v0[5]),
                      pack_bf16x2(v0[6], v0[7])};
    const u32x4 p1 = {pack_bf16x2(v1[0], v1[1]), pack_bf16x2(v1[2], v1[3]), pack_bf16x2(v1[4], v1[5]),
                      pack_bf16x2(v1[6], v1[7])};
    wb[nt][0] = __builtin_bit_cast(bf16x8, p0);
    wb[nt][1] = __builtin_bit_cast(bf16x8, p1);
  }
}

__device__ __forceinline__ int cf_tap_shift(int tap, int W) { return (tap / 3 - 1) * W + tap % 3 - 1; }

// image index of position `pos` of the chunk (the centre tap)
__device__ __forceinline__ int cf_image_row(int pos, int logF) {
  const int F = 1 << logF;
  return ((pos >> logF) + 1) * (F + 2) + (pos & (F - 1)) + 1;
}

// xp[nt][jp] = the bf16 pair round_bf16(conv3x3(in, w)) at positions 16 tile + 4 g + 2 jp (low half) and + 1 (high half),
// channel 4 c + nt: THE value of x1 everywhere (fp32 accumulation in the MFMA's fixed order, one rounding)
struct CfLane {                             // what a lane needs of the geometry, computed once per kernel
  int xr[kCfTiles / 4];                     // image row of its A-operand position in each of the wave's tiles
  int row[kCfTiles / 4];                    // time row of the tile within the chunk
  int pooled[kCfTiles / 4];                 // element offset of its pooled outputs within the chunk's part of y / dy
  int sh0, sh1, sh8;                        // image offsets of taps 2 g, 2 g + 1 and 8
  bool g0;
};

__device__ __forceinline__ CfLane cf_lane(int logF, int lane, int wave) {
  CfLane ln;
  const int W = (1 << logF) + 2, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < kCfTiles / 4; ++i) {
    const int pos = (wave + 4 * i) * 16;
    ln.xr[i] = cf_image_row(pos + (lane & 15), logF);
    ln.row[i] = pos >> logF;
    ln.pooled[i] = ((pos + 4 * g) >> 1) * kCfCout + 4 * (lane & 15);
  }
  ln.sh0 = cf_tap_shift(2 * g, W);
  ln.sh1 = cf_tap_shift(2 * g + 1, W);
  ln.sh8 = W + 1;
  ln.g0 = g == 0;
  return ln;
}

__device__ __forceinline__ void cf_conv_tile(const uint2* img, const CfLane& ln, int i, const bf16x8 (&wb)[4][2],
                                             unsigned (&xp)[4][2]) {
  const int xr = ln.xr[i];
  const uint2 t0 = img[xr + ln.sh0], t1 = img[xr + ln.sh1];
  uint2 t8 = img[xr + ln.sh8];
  if (!ln.g0) t8 = make_uint2(0u, 0u);
  const u32x4 p0 = {t0.x, t0.y, t1.x, t1.y}, p1 = {t8.x, t8.y, 0u, 0u};
  const bf16x8 a0 = __builtin_bit_cast(bf16x8, p0), a1 = __builtin_bit_cast(bf16x8, p1);
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wb[nt][0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wb[nt][1], acc, 0, 0, 0);
    xp[nt][0] = pack_bf16x2(acc[0], acc[1]);
    xp[nt][1] = pack_bf16x2(acc[2], acc[3]);
  }
}

// The packed pairs of two tiles are, as they stand, an MFMA operand with K = the wave's 32 positions: lane (g, c)
// holds 8 positions (k = 8 g + e: tile e / 4, position 4 g + e % 4) of channel 4 c + nt -- row c of an A operand
// (channels x positions) and column c of a B operand (positions x channels) alike.  Sums over positions are therefore
// matrix products, which cost no vector-ALU time: ones * X = column sums, X^T X = sums of squares on the diagonal.
__device__ __forceinline__ bf16x8 cf_operand(const unsigned (&t0)[2], const unsigned (&t1)[2]) {
  const u32x4 v = {t0[0], t0[1], t1[0], t1[1]};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 cf_ones() {
  const u32x4 v = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
  return __builtin_bit_cast(bf16x8, v);
}

// relu of a packed bf16 pair as 16-bit integers (a negative float has the sign bit); the results are non-negative
// floats, whose order is the order of their bit patterns
__device__ __forceinline__ unsigned cf_relu_pair(unsigned p) {
  const s16x2 v = __builtin_bit_cast(s16x2, p), zero = {0, 0};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(v, zero));
}

// relu(round_bf16(a x + b)) of both bins of a pooling pair (tail_apply_kernel<bf16, 2> / route<bf16, 2>), packed
__device__ __forceinline__ unsigned cf_activate(unsigned xpair, float a, float b) {
  return cf_relu_pair(pack_bf16x2(fmaf(bf16_lo(xpair), a, b), fmaf(bf16_hi(xpair), a, b)));
}

struct CfChunk {
  int b, t0;
};

__device__ __forceinline__ CfChunk cf_chunk(const CfGeom& gm, int chunk) {
  CfChunk c;
  c.b = chunk / gm.chunks_per_clip;
  c.t0 = (chunk - c.b * gm.chunks_per_clip) * (kCfPos >> gm.logF);
  return c;
}

// rows t0-1 .. t0+TC of the clip -> registers (zero outside [0, T)); piece = one position's 4 channels
__device__ __forceinline__ void cf_load_image(const uint2* in, const CfGeom& gm, const CfChunk& c, uint2 (&r)[kCfStage]) {
  const int pieces = ((kCfPos >> gm.logF) + 2) << gm.logF;
#pragma unroll
  for (int i = 0; i < kCfStage; ++i) {
    const int p = threadIdx.x + i * kCfThreads;
    const int t = c.t0 - 1 + (p >> gm.logF);
    r[i] = make_uint2(0u, 0u);
    if (p < pieces && t >= 0 && t < gm.T)
      r[i] = in[((static_cast<long>(c.b) * gm.T + t) << gm.logF) + (p & ((1 << gm.logF) - 1))];
  }
}

__device__ __forceinline__ void cf_store_image(uint2* img, const CfGeom& gm, const uint2 (&r)[kCfStage]) {
  const int F = 1 << gm.logF, pieces = ((kCfPos >> gm.logF) + 2) << gm.logF;
#pragma unroll
  for (int i = 0; i < kCfStage; ++i) {
    const int p = threadIdx.x + i * kCfThreads;
    if (p < pieces) img[(p >> gm.logF) * (F + 2) + (p & (F - 1)) + 1] = r[i];
  }
}

// the wave's tiles of a chunk, i = 0 .. 3 (tile wave + 4 i), taken as two pairs h of two tiles u: i = 2 h + u
__device__ __forceinline__ bool cf_tile_valid(const CfGeom& gm, const CfChunk& c, const CfLane& ln, int i) {
  return c.t0 + ln.row[i] < gm.T;                                // (wave-uniform)
}

// element offset of the chunk's first pooled output in y / dy ([B][T][F/2][64]); a lane's are + ln.pooled[i] + 64 jp
__device__ __forceinline__ long cf_pooled_base(const CfGeom& gm, const CfChunk& c) {
  return (((static_cast<long>(c.b) * gm.T + c.t0) << gm.logF) >> 1) * kCfCout;
}

__device__ __forceinline__ float cf_pick(const f32x4& v, int j) {
  return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3];
}

// per-wave accumulators -> this workgroup's partial row.  colsum[nt]: every row holds the column sums (channel 4 c + nt
// in column c); diag[nt]: the statistic of channel 4 c + nt is element (c, c), held by lane group c / 4 at j = c % 4.
// The four waves are added in wave order.
__device__ __forceinline__ void cf_block_partials(const f32x4 (&colsum)[4], const f32x4 (&diag)[4], float* part /* [4 * 128] */,
                                                  float* __restrict__ partials, int nrows) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (g == 0) part[wave * 128 + 4 * c + nt] = colsum[nt][0];
    if (g == (c >> 2)) part[wave * 128 + 64 + 4 * c + nt] = cf_pick(diag[nt], c & 3);
  }
  __syncthreads();
  if (tid < 2 * kCfCout) {
    const int s = tid >> 6, ch = tid & 63;
    const float sum = ((part[tid] + part[128 + tid]) + part[256 + tid]) + part[384 + tid];
    partials[(static_cast<long>(s) * nrows + blockIdx.x) * kCfCout + ch] = sum;
  }
}

// The statistics kernel's partial row: the column sums as above; the sums of squares arrive as doubles (lane group c / 4
// holds channel 4 c + nt), are added in wave order in double and stored as a float pair hi + lo in planes 1 and 2.
__device__ __forceinline__ void cf_stats_partials(const f32x4 (&colsum)[4], const double (&sq)[4], float* part /* [4 * 64] */,
                                                  double* partd /* [4 * 64] */, float* __restrict__ partials, int nrows) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    if (g == 0) part[wave * kCfCout + 4 * c + nt] = colsum[nt][0];
    if (g == (c >> 2)) partd[wave * kCfCout + 4 * c + nt] = sq[nt];
  }
  __syncthreads();
  if (tid < kCfCout) {
    const float sum = ((part[tid] + part[kCfCout + tid]) + part[2 * kCfCout + tid]) + part[3 * kCfCout + tid];
    const double sumsq = ((partd[tid] + partd[kCfCout + tid]) + partd[2 * kCfCout + tid]) + partd[3 * kCfCout + tid];
    const float hi = static_cast<float>(sumsq), lo = static_cast<float>(sumsq - static_cast<double>(hi));
    const long row = static_cast<long>(blockIdx.x) * kCfCout + tid, plane = static_cast<long>(nrows) * kCfCout;
    partials[row] = sum;
    partials[plane + row] = hi;
    partials[2 * plane + row] = lo;
  }
}

// The finalise launches: block cg reduces the partial rows of channels 8 cg .. 8 cg + 7 (both statistics) in double in a
// fixed order -- 16 row subsets, then the subsets in order -- and thread ch < 8 finishes its channel.  (Reducing the rows
// in the prologue of every workgroup of the next kernel instead was measured: 256 - 512 workgroups each pulling the
// 128 - 256 KB of partials through L2 cost that kernel 6 - 8 us, a launch of this costs 2 - 3.)
constexpr int kCfFinalThreads = 256;

// (kLowPlane: the second statistic is a float pair, its low halves in plane 2 -- cf_stats_partials)
template <bool kLowPlane>
__device__ __forceinline__ void cf_final_sums(const float* __restrict__ partials, int nrows, double* red /* [16 * 16] */) {
  const int tid = threadIdx.x, item = tid & 15, s = item >> 3, ch = blockIdx.x * 8 + (item & 7), rg = tid >> 4;
  double sum = 0.0;
#pragma unroll 8
  for (int r = rg; r < nrows; r += 16) {
    sum += static_cast<double>(partials[(static_cast<long>(s) * nrows + r) * kCfCout + ch]);
    if (kLowPlane && s == 1) sum += static_cast<double>(partials[(2L * nrows + r) * kCfCout + ch]);
  }
  red[rg * 16 + item] = sum;
  __syncthreads();
  if (tid < 16) {
    for (int k = 1; k < 16; ++k) sum += red[k * 16 + tid];
    red[tid] = sum;
  }
  __syncthreads();
}

// tail_stats_final_kernel of convtail.hip (training mode), from unshifted sums
__global__ __launch_bounds__(kCfFinalThreads) void convfirst_stats_final_kernel(
    const float* __restrict__ partials, int nrows, long rows, const float* __restrict__ weight,
    const float* __restrict__ bias, float* __restrict__ running_mean, float* __restrict__ running_var, float momentum,
    float eps, float* __restrict__ mean_invstd, float* __restrict__ scale_shift) {
  __shared__ double red[16 * 16];
  cf_final_sums<true>(partials, nrows, red);
  if (threadIdx.x < 8) {
    const int ch = blockIdx.x * 8 + threadIdx.x;
    const double n = static_cast<double>(rows);
    const double mean = red[threadIdx.x] / n;
    double var = red[8 + threadIdx.x] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const double unbiased = rows > 1 ? var * n / (n - 1.0) : var;
    running_mean[ch] = static_cast<float>((1.0 - momentum) * running_mean[ch] + momentum * mean);
    running_var[ch] = static_cast<float>((1.0 - momentum) * running_var[ch] + momentum * unbiased);
    const float meanf = static_cast<float>(mean);
    const float invstd = static_cast<float>(1.0 / sqrt(var + static_cast<double>(eps)));
    // two roundings (the fp32 invstd, then the product): up to 1.5 ulp from weight / sigma, so up to 1 ulp from the `a` of
    // csrc/convtail.hip, which rounds weight * the double invstd once; tests/test_convfirst_parity_gpu.py pins this
    // path's `a` to fl32(weight * the returned invstd) bit for bit and the invstd to the float64 value
    const float a = weight[ch] * invstd;
    mean_invstd[ch] = meanf;
    mean_invstd[kCfCout + ch] = invstd;
    scale_shift[ch] = a;
    scale_shift[kCfCout + ch] = bias[ch] - meanf * a;
  }
}

// tail_bwd_final_kernel of convtail.hip, with sum dz (x - mean) = sum dz x - mean sum dz formed here in double
__global__ __launch_bounds__(kCfFinalThreads) void convfirst_bwd_final_kernel(
    const float* __restrict__ partials, int nrows, long rows, const float* __restrict__ mean_invstd,
    const float* __restrict__ scale_shift, float* __restrict__ dgamma, float* __restrict__ dbeta,
    float* __restrict__ coef /* [2][64] p, q */) {
  __shared__ double red[16 * 16];
  cf_final_sums<false>(partials, nrows, red);
  if (threadIdx.x < 8) {
    const int ch = blockIdx.x * 8 + threadIdx.x;
    const double invstd = mean_invstd[kCfCout + ch], mean = mean_invstd[ch], a = scale_shift[ch];
    const double s_dz = red[threadIdx.x], s_dzx = (red[8 + threadIdx.x] - mean * s_dz) * invstd;      // sum dz xhat
    const double n = static_cast<double>(rows);
    dbeta[ch] = static_cast<float>(s_dz);
    dgamma[ch] = static_cast<float>(s_dzx);
    const double q = -a * (s_dzx / n) * invstd;
    coef[ch] = static_cast<float>(-a * (s_dz / n) - q * mean);
    coef[kCfCout + ch] = static_cast<float>(q);
  }
}

#define SELD_CF_PROLOGUE()                                                                   \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                             \
  const uint2* const in2 = static_cast<const uint2*>(in);                                    \
  for (int i = tid; i < kCfImage; i += kCfThreads) img[i] = make_uint2(0u, 0u);              \
  const CfLane ln = cf_lane(gm.logF, lane, wave)

// ------------------------------------------------------------------------------------------------ 1: statistics
// sum x and sum x^2 per channel.  The products x * x of bf16 values are exact in fp32; each matrix instruction adds the
// squares of 32 positions into a ZERO accumulator and its diagonal is then added up in double, in the wave, across the
// waves and across the workgroups, so the only fp32 roundings a square passes through are those inside one instruction:
// invstd stays within an ulp of the float64 value even when a single chunk leaves nothing to average over (a chained fp32
// accumulator was 1.09 ulp off there), and no shift is needed to keep E[x^2] - E[x]^2 from cancelling.
__global__ __launch_bounds__(kCfThreads, 2) void convfirst_stats_kernel(const void* __restrict__ in, CfWeights w, CfGeom gm,
                                                                        float* __restrict__ partials) {
  __shared__ uint2 img[kCfImage];
  __shared__ float part[4 * kCfCout];
  __shared__ double partd[4 * kCfCout];
  SELD_CF_PROLOGUE();
  f32x4 colsum[4];
  double sq[4];                                                  // channel 4 c + nt, valid in lane group c / 4
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    colsum[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    sq[nt] = 0.0;
  }
  const bf16x8 ones = cf_ones();
  const int dj = lane & 3;                                       // the diagonal element (c, c) is j = c % 4 of group c / 4
  uint2 rin[kCfStage];
  int chunk = blockIdx.x;
  if (chunk < gm.chunks) cf_load_image(in2, gm, cf_chunk(gm, chunk), rin);
  bf16x8 wb[4][2];
  cf_load_weights(w, lane, wb);
  for (; chunk < gm.chunks; chunk += gridDim.x) {
    const CfChunk c = cf_chunk(gm, chunk);
    __syncthreads();                                             // the previous chunk's image reads are done
    cf_store_image(img, gm, rin);
    __syncthreads();
    if (chunk + static_cast<int>(gridDim.x) < gm.chunks) cf_load_image(in2, gm, cf_chunk(gm, chunk + gridDim.x), rin);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned xp[2][4][2] = {};
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (cf_tile_valid(gm, c, ln, 2 * h + u)) cf_conv_tile(img, ln, 2 * h + u, wb, xp[u]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 x = cf_operand(xp[0][nt], xp[1][nt]);
        colsum[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, x, colsum[nt], 0, 0, 0);
        const f32x4 diag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, x, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
        sq[nt] += static_cast<double>(cf_pick(diag, dj));
      }
    }
  }
  cf_stats_partials(colsum, sq, part, partd, partials, gridDim.x);
}

// ------------------------------------------------------------------------------------------------ 2: apply
__global__ __launch_bounds__(kCfThreads, 2) void convfirst_apply_kernel(const void* __restrict__ in, CfWeights w, CfGeom gm,
                                                                        const float* __restrict__ scale_shift,
                                                                        unsigned short* __restrict__ y) {
  __shared__ uint2 img[kCfImage];
  SELD_CF_PROLOGUE();
  uint2 rin[kCfStage];
  int chunk = blockIdx.x;
  if (chunk < gm.chunks) cf_load_image(in2, gm, cf_chunk(gm, chunk), rin);
  bf16x8 wb[4][2];
  cf_load_weights(w, lane, wb);
  float a[4], b[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    a[nt] = scale_shift[4 * (lane & 15) + nt];
    b[nt] = scale_shift[kCfCout + 4 * (lane & 15) + nt];
  }
  for (; chunk < gm.chunks; chunk += gridDim.x) {
    const CfChunk c = cf_chunk(gm, chunk);
    __syncthreads();
    cf_store_image(img, gm, rin);
    __syncthreads();
    if (chunk + static_cast<int>(gridDim.x) < gm.chunks) cf_load_image(in2, gm, cf_chunk(gm, chunk + gridDim.x), rin);
#pragma unroll
    for (int i = 0; i < kCfTiles / 4; ++i) {
      if (!cf_tile_valid(gm, c, ln, i)) continue;
      unsigned xp[4][2];
      cf_conv_tile(img, ln, i, wb, xp);
      const long o = cf_pooled_base(gm, c) + ln.pooled[i];
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        unsigned m[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {                         // max(relu(z0), relu(z1)): non-negative, integer order
          const unsigned z = cf_activate(xp[nt][jp], a[nt], b[nt]);
          m[nt] = max(z & 0xffffu, z >> 16);
        }
        *reinterpret_cast<uint2*>(y + o + jp * kCfCout) = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
      }
    }
  }
}

// the lane's dy of the chunk's tiles wave, wave + 4, ..: [tile][pooled pair] x 4 channels
__device__ __forceinline__ void cf_load_dy(const unsigned short* dy, const CfGeom& gm, const CfChunk& c, const CfLane& ln,
                                           uint2 (&r)[kCfTiles / 4][2]) {
  const unsigned short* const base = dy + cf_pooled_base(gm, c);
#pragma unroll
  for (int i = 0; i < kCfTiles / 4; ++i) {
    const bool valid = cf_tile_valid(gm, c, ln, i);
    const unsigned short* const o = base + ln.pooled[i];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      r[i][jp] = make_uint2(0u, 0u);
      if (valid) r[i][jp] = *reinterpret_cast<const uint2*>(o + jp * kCfCout);
    }
  }
}

// ------------------------------------------------------------------------------------------------ 3: backward reduce
// sum dz and sum dz x per channel (dz = dy routed to the bin that won the pooling, if the ReLU passed it: a bf16 value,
// so both sums are again matrix products); the finalisation forms sum dz (x - mean) = sum dz x - mean sum dz in double.
__global__ __launch_bounds__(kCfThreads, 2) void convfirst_bwd_reduce_kernel(
    const void* __restrict__ in, CfWeights w, CfGeom gm, const unsigned short* __restrict__ dy,
    const float* __restrict__ scale_shift, float* __restrict__ partials) {
  __shared__ uint2 img[kCfImage];
  __shared__ float part[4 * 128];
  SELD_CF_PROLOGUE();
  float a[4], b[4];
  f32x4 colsum[4], diag[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    a[nt] = scale_shift[4 * (lane & 15) + nt];
    b[nt] = scale_shift[kCfCout + 4 * (lane & 15) + nt];
    colsum[nt] = diag[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  const bf16x8 ones = cf_ones();
  uint2 rin[kCfStage], rdy[kCfTiles / 4][2];
  int chunk = blockIdx.x;
  if (chunk < gm.chunks) {
    cf_load_image(in2, gm, cf_chunk(gm, chunk), rin);
    cf_load_dy(dy, gm, cf_chunk(gm, chunk), ln, rdy);
  }
  bf16x8 wb[4][2];
  cf_load_weights(w, lane, wb);
  for (; chunk < gm.chunks; chunk += gridDim.x) {
    const CfChunk c = cf_chunk(gm, chunk);
    __syncthreads();
    cf_store_image(img, gm, rin);
    uint2 g2[kCfTiles / 4][2];
#pragma unroll
    for (int i = 0; i < kCfTiles / 4; ++i) {
      g2[i][0] = rdy[i][0];
      g2[i][1] = rdy[i][1];
    }
    __syncthreads();
    if (chunk + static_cast<int>(gridDim.x) < gm.chunks) {
      cf_load_image(in2, gm, cf_chunk(gm, chunk + gridDim.x), rin);
      cf_load_dy(dy, gm, cf_chunk(gm, chunk + gridDim.x), ln, rdy);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned xp[2][4][2] = {}, dz[2][4][2] = {};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!cf_tile_valid(gm, c, ln, 2 * h + u)) continue;
        cf_conv_tile(img, ln, 2 * h + u, wb, xp[u]);
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          const uint2 gw = g2[2 * h + u][jp];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {                       // route<bf16, 2>: first bin wins ties, ReLU gate
            const unsigned z = cf_activate(xp[u][nt][jp], a[nt], b[nt]);
            const unsigned word = nt < 2 ? gw.x : gw.y;
            const unsigned to_lo = (nt & 1) ? word >> 16 : word & 0xffffu;
            const unsigned to_hi = (nt & 1) ? word & 0xffff0000u : word << 16;
            dz[u][nt][jp] = z == 0u ? 0u : ((z >> 16) > (z & 0xffffu) ? to_hi : to_lo);
          }
        }
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 x = cf_operand(xp[0][nt], xp[1][nt]), d = cf_operand(dz[0][nt], dz[1][nt]);
        colsum[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, d, colsum[nt], 0, 0, 0);
        diag[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(d, x, diag[nt], 0, 0, 0);
      }
    }
  }
  cf_block_partials(colsum, diag, part, partials, gridDim.x);
}

// ------------------------------------------------------------------------------------------------ 4: weight gradient
__device__ __forceinline__ s16x4 cf_tr_read(const unsigned short* base, int offset_shorts) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + offset_shorts));
}
__device__ __forceinline__ bf16x8 cf_join(s16x4 lo, s16x4 hi) {
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// dx1 = a dz + p + q x (tail_bwd_apply_kernel<bf16, 2>), rounded to bf16, is once more an A operand as it leaves the
// vector ALU (channels x the wave's 32 positions); B = the (tap, ci) columns of the same positions, read from the image
// with ds_read_b64_tr_b16 as in convwgrad.hip: lane 4 qq + pp of the 16-lane group g supplies position 4 g + qq of the
// tile, columns 4 pp .. 4 pp + 3 = tap 4 nb + pp, and receives column lane & 15 of positions 4 g .. 4 g + 3.
__global__ __launch_bounds__(kCfThreads, 2) void convfirst_wgrad_kernel(
    const void* __restrict__ in, CfWeights w, CfGeom gm, const unsigned short* __restrict__ dy,
    const float* __restrict__ scale_shift, const float* __restrict__ coef, float* __restrict__ slots) {
  __shared__ uint2 img[kCfImage];
  SELD_CF_PROLOGUE();
  uint2 rin[kCfStage], rdy[kCfTiles / 4][2];
  int chunk = blockIdx.x;
  if (chunk < gm.chunks) {
    cf_load_image(in2, gm, cf_chunk(gm, chunk), rin);
    cf_load_dy(dy, gm, cf_chunk(gm, chunk), ln, rdy);
  }
  bf16x8 wb[4][2];
  cf_load_weights(w, lane, wb);
  float a[4], b[4], p[4], q[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int ch = 4 * (lane & 15) + nt;
    a[nt] = scale_shift[ch];
    b[nt] = scale_shift[kCfCout + ch];
    p[nt] = coef[ch];
    q[nt] = coef[kCfCout + ch];
  }
  const int W = (1 << gm.logF) + 2, g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
  int tap_shift[3];
#pragma unroll
  for (int nb = 0; nb < 3; ++nb) tap_shift[nb] = cf_tap_shift(min(4 * nb + pp, 8), W);      // columns >= 36: never stored
  int xb[kCfTiles / 4];                                          // image row of the lane's B-operand position per tile
#pragma unroll
  for (int i = 0; i < kCfTiles / 4; ++i) xb[i] = cf_image_row((wave + 4 * i) * 16 + 4 * g + qq, gm.logF);
  f32x4 acc[4][3];                                               // [channel set nt][column tile nb]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int nb = 0; nb < 3; ++nb) acc[nt][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const unsigned short* const imgs = reinterpret_cast<const unsigned short*>(img);

  for (; chunk < gm.chunks; chunk += gridDim.x) {
    const CfChunk c = cf_chunk(gm, chunk);
    __syncthreads();                                             // the previous chunk's image reads are done
    cf_store_image(img, gm, rin);
    uint2 g2[kCfTiles / 4][2];
#pragma unroll
    for (int i = 0; i < kCfTiles / 4; ++i) {
      g2[i][0] = rdy[i][0];
      g2[i][1] = rdy[i][1];
    }
    __syncthreads();
    if (chunk + static_cast<int>(gridDim.x) < gm.chunks) {
      cf_load_image(in2, gm, cf_chunk(gm, chunk + gridDim.x), rin);
      cf_load_dy(dy, gm, cf_chunk(gm, chunk + gridDim.x), ln, rdy);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned dxp[2][4][2] = {};                                // rows past the clip: zero gradient
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!cf_tile_valid(gm, c, ln, 2 * h + u)) continue;
        unsigned xp[4][2];
        cf_conv_tile(img, ln, 2 * h + u, wb, xp);
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          const uint2 gw = g2[2 * h + u][jp];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const unsigned z = cf_activate(xp[nt][jp], a[nt], b[nt]);
            const unsigned word = nt < 2 ? gw.x : gw.y;
            const float gv = (nt & 1) ? bf16_hi(word) : bf16_lo(word);
            const bool pass = z != 0u, second = (z >> 16) > (z & 0xffffu);
            const float g0 = (pass && !second) ? gv : 0.0f, g1 = (pass && second) ? gv : 0.0f;
            const float d0 = fmaf(a[nt], g0, fmaf(q[nt], bf16_lo(xp[nt][jp]), p[nt]));
            const float d1 = fmaf(a[nt], g1, fmaf(q[nt], bf16_hi(xp[nt][jp]), p[nt]));
            dxp[u][nt][jp] = pack_bf16x2(d0, d1);
          }
        }
      }
      const int xr0 = xb[2 * h], xr1 = xb[2 * h + 1];
      bf16x8 bf[3];
#pragma unroll
      for (int nb = 0; nb < 3; ++nb)
        bf[nb] = cf_join(cf_tr_read(imgs, (xr0 + tap_shift[nb]) * kCfCin), cf_tr_read(imgs, (xr1 + tap_shift[nb]) * kCfCin));
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const bf16x8 af = cf_operand(dxp[0][nt], dxp[1][nt]);
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) acc[nt][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[nb], acc[nt][nb], 0, 0, 0);
      }
    }
  }
  // C/D of a 16x16 tile: column (tap, ci) = 16 nb + (lane & 15), row 4 g + j = channel 4 (4 g + j) + nt.  The four
  // waves add their tiles in wave order through LDS, then the slot is written coalesced.
  __syncthreads();
  __shared__ float tile[kCfCout * kCfK];
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int nb = 0; nb < 3; ++nb) {
          const int n = nb * 16 + (lane & 15);
          if (n < kCfK)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float* const e = tile + (4 * (4 * g + j) + nt) * kCfK + n;
              *e = wv == 0 ? acc[nt][nb][j] : *e + acc[nt][nb][j];
            }
        }
    }
    __syncthreads();
  }
  float* const slot = slots + static_cast<long>(blockIdx.x) * kCfCout * kCfK;
  for (int i = tid; i < kCfCout * kCfK; i += kCfThreads) slot[i] = tile[i];
}

// dw[co][ci][r][s] (the parameter's strides and dtype) = sum over the slots, fixed order: thread row r adds slots
// r, r + 16, .. of 4 consecutive elements (one tap's 4 input channels), then row 0 adds the 16 row sums in order
__global__ __launch_bounds__(kCfSumThreads) void convfirst_wgrad_sum_kernel(const float* __restrict__ slots, int nslots,
                                                                            void* __restrict__ dw, int dw_is_bf16, long sco,
                                                                            long sci, long sr, long ss) {
  constexpr int kCols = kCfSumThreads / kCfSumRows;
  constexpr int kCount = kCfCout * kCfK;
  __shared__ float4 part[kCfSumRows][kCols];
  const int col = threadIdx.x % kCols, row = threadIdx.x / kCols;
  const int i = (blockIdx.x * kCols + col) * 4;
  float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < kCount)
    for (int k = row; k < nslots; k += kCfSumRows) {
      const float4 v = *reinterpret_cast<const float4*>(slots + static_cast<long>(k) * kCount + i);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  part[row][col] = s;
  __syncthreads();
  if (row != 0 || i >= kCount) return;
#pragma unroll
  for (int r = 1; r < kCfSumRows; ++r) {
    const float4 v = part[r][col];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const int co = i / kCfK, tap = (i - co * kCfK) >> 2;
  const long o = co * sco + (tap / 3) * sr + (tap % 3) * ss;
  const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int ci = 0; ci < kCfCin; ++ci) {
    if (dw_is_bf16) static_cast<unsigned short*>(dw)[o + ci * sci] = bf16_bits(v[ci]);
    else static_cast<float*>(dw)[o + ci * sci] = v[ci];
  }
}

#undef SELD_CF_PROLOGUE

bool cf_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return Cin == kCfCin && Cout == kCfCout && (F == 16 || F == 32 || F == 64 || F == 128 || F == 256);
}

int cf_geometry(const char* who, int64_t B, int64_t T, int64_t F, CfGeom* gm) {
  if (B <= 0 || T <= 0) return fail(kErrInvalidArgument, std::string(who) + ": B and T must be positive");
  if (!cf_supported(F, kCfCin, kCfCout)) return fail(kErrUnsupported, std::string(who) + ": F must be 16, 32, 64, 128 or 256");
  int logF = 4;
  while ((1 << logF) < F) ++logF;
  const int tc = kCfPos >> logF;
  const int64_t per_clip = (T + tc - 1) / tc;
  if (B * per_clip > (1 << 30) || B * T * F > (1LL << 40)) return fail(kErrUnsupported, std::string(who) + ": tensor too large");
  gm->T = static_cast<int>(T);
  gm->logF = logF;
  gm->chunks_per_clip = static_cast<int>(per_clip);
  gm->chunks = static_cast<int>(B * per_clip);
  gm->rows = B * T * F;
  return kOk;
}

int cf_groups(const DeviceState* st, const CfGeom& gm) {
  int groups = 2 * (st->num_cus > 0 ? st->num_cus : 256);
  if (groups > kCfMaxGroups) groups = kCfMaxGroups;
  return groups < gm.chunks ? groups : gm.chunks;
}

bool cf_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int cf_packed(const void* w, int is_bf16, int64_t sco, int64_t sci, int64_t sr, int64_t ss) {
  return is_bf16 && sci == 1 && ss == kCfCin && sr == 3 * kCfCin && sco == kCfK && cf_aligned(w, 8) ? 1 : 0;
}

}  // namespace

}  // namespace seld

extern "C" {

int seld_convfirst_supported(int64_t F, int64_t Cin, int64_t Cout) { return seld::cf_supported(F, Cin, Cout) ? 1 : 0; }

int64_t seld_convfirst_workspace_floats(int backward) {
  using namespace seld;
  const int64_t partials = 3LL * kCfMaxGroups * kCfCout;      // forward: sum, sum of squares as a float pair
  return backward ? partials + static_cast<int64_t>(kCfMaxGroups) * kCfCout * kCfK + 2 * kCfCout : partials;
}

int seld_convfirst_forward(const void* in, const void* w, int w_is_bf16, int64_t w_sco, int64_t w_sci, int64_t w_sr,
                           int64_t w_ss, int64_t B, int64_t T, int64_t F, const float* bn_weight, const float* bn_bias,
                           float* running_mean, float* running_var, float momentum, float eps, void* y,
                           float* mean_invstd, float* scale_shift, float* workspace, int phases, void* stream_) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  CfGeom gm;
  if (int rc = cf_geometry("seld_convfirst_forward", B, T, F, &gm)) return rc;
  if (!in || !w || !bn_weight || !bn_bias || !running_mean || !running_var || !y || !mean_invstd || !scale_shift || !workspace)
    return fail(kErrInvalidArgument, "seld_convfirst_forward: null pointer");
  if (!cf_aligned(in, 8) || !cf_aligned(y, 8) || !cf_aligned(workspace, 16))
    return fail(kErrInvalidArgument, "seld_convfirst_forward: in / y 8-byte, workspace 16-byte aligned required");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const CfWeights cw{w, w_is_bf16, cf_packed(w, w_is_bf16, w_sco, w_sci, w_sr, w_ss), static_cast<long>(w_sco), static_cast<long>(w_sci), static_cast<long>(w_sr), static_cast<long>(w_ss)};
  const int groups = cf_groups(st, gm);
  if (phases & 1)
    hipLaunchKernelGGL(convfirst_stats_kernel, dim3(groups), dim3(kCfThreads), 0, stream, in, cw, gm, workspace);
  if (phases & 2) {
    hipLaunchKernelGGL(convfirst_stats_final_kernel, dim3(kCfCout / 8), dim3(kCfFinalThreads), 0, stream, workspace, groups,
                       gm.rows, bn_weight, bn_bias, running_mean, running_var, momentum, eps, mean_invstd, scale_shift);
    hipLaunchKernelGGL(convfirst_apply_kernel, dim3(groups), dim3(kCfThreads), 0, stream, in, cw, gm, scale_shift,
                       static_cast<unsigned short*>(y));
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

int seld_convfirst_backward(const void* in, const void* w, int w_is_bf16, int64_t w_sco, int64_t w_sci, int64_t w_sr,
                            int64_t w_ss, const void* dy, int64_t B, int64_t T, int64_t F, const float* mean_invstd,
                            const float* scale_shift, void* dw, int dw_is_bf16, int64_t dw_sco, int64_t dw_sci,
                            int64_t dw_sr, int64_t dw_ss, float* dgamma, float* dbeta, float* workspace, int phases,
                            void* stream_) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  CfGeom gm;
  if (int rc = cf_geometry("seld_convfirst_backward", B, T, F, &gm)) return rc;
  if (!in || !w || !dy || !mean_invstd || !scale_shift || !dw || !dgamma || !dbeta || !workspace)
    return fail(kErrInvalidArgument, "seld_convfirst_backward: null pointer");
  if (!cf_aligned(in, 8) || !cf_aligned(dy, 8) || !cf_aligned(workspace, 16))
    return fail(kErrInvalidArgument, "seld_convfirst_backward: in / dy 8-byte, workspace 16-byte aligned required");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const CfWeights cw{w, w_is_bf16, cf_packed(w, w_is_bf16, w_sco, w_sci, w_sr, w_ss), static_cast<long>(w_sco), static_cast<long>(w_sci), static_cast<long>(w_sr), static_cast<long>(w_ss)};
  const int groups = cf_groups(st, gm);
  float* const slots = workspace + 2L * kCfMaxGroups * kCfCout;
  float* const coef = slots + static_cast<long>(kCfMaxGroups) * kCfCout * kCfK;
  const unsigned short* const g = static_cast<const unsigned short*>(dy);
  if (phases & 1)
    hipLaunchKernelGGL(convfirst_bwd_reduce_kernel, dim3(groups), dim3(kCfThreads), 0, stream, in, cw, gm, g, scale_shift,
                       workspace);
  if (phases & 2) {
    hipLaunchKernelGGL(convfirst_bwd_final_kernel, dim3(kCfCout / 8), dim3(kCfFinalThreads), 0, stream, workspace, groups,
                       gm.rows, mean_invstd, scale_shift, dgamma, dbeta, coef);
    hipLaunchKernelGGL(convfirst_wgrad_kernel, dim3(groups), dim3(kCfThreads), 0, stream, in, cw, gm, g, scale_shift, coef,
                       slots);
    constexpr int kCols = kCfSumThreads / kCfSumRows;
    hipLaunchKernelGGL(convfirst_wgrad_sum_kernel, dim3((kCfCout * kCfK / 4 + kCols - 1) / kCols), dim3(kCfSumThreads), 0,
                       stream, slots, groups, dw, dw_is_bf16, static_cast<long>(dw_sco), static_cast<long>(dw_sci),
                       static_cast<long>(dw_sr), static_cast<long>(dw_ss));
  }
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
