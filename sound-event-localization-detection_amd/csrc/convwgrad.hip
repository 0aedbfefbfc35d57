// Weight gradient of the encoder's 3x3 / stride 1 / pad 1 / bias-free convolutions (model_crnn.py:5-17, ConvBlock.conv;
// the Conformer's encoder is the same code) on channels-last bf16 activations.
//
//   dW[co][r][s][ci] = sum over (b, t, f) of dy[b][t][f][co] * x[b][t + r - 1][f + s - 1][ci]   (zero outside the map)
//
// is a GEMM with M = Cout, N = 9 * Cin and a very long K = B * T * F.  The library's solvers reach 70-620 TFLOP/s on the
// encoder's shapes and finish with a split-K that adds with atomics into a zero-filled fp32 workspace, then a cast and
// a copy.  Here:
//
//   * a workgroup (8 waves, 2 co x 4 ci) owns a 64-co x 64-ci tile for all nine taps and a K slab: a run of chunks, a
//     chunk being kWgKc positions = TC consecutive time rows of one clip.  Per chunk it stages dy [kWgKc][64 co] and the
//     x rows t0-1 .. t0+TC with zero rows outside [0, T) and a zero column on each frequency edge, [TC+2][F+2][64 ci],
//     in LDS once; the nine taps are nine shifted views of that x image (a constant row offset per tap).
//   * both operands are position-major in memory (channels innermost), so the MFMA fragments, 8 positions of one
//     channel, come from ds_read_b64_tr_b16.  A K-group of 32 positions is read as two 4-row halves; the MFMA's k
//     numbering is a free relabelling of positions as long as both operands use the same one, so lanes 16g..16g+15
//     take positions 4g..4g+3 and 16+4g..16+4g+3: a 32-lane half then reads 8 consecutive LDS rows, which the 160-byte
//     row pitch spreads over all 64 banks (conflict-free).
//   * v_mfma_f32_16x16x32_bf16; a wave owns 32 co x 16 ci: fp32 accumulators for 9 taps x 2 tiles (72 registers), two
//     dy fragments per K-group reused by all nine taps, one x fragment per tap.
//   * ONE workgroup per CU on HALF of its registers: at most 128 per lane and no scratch
//     (tests/test_conv_wgrad_occupancy_cpu.py), so its two waves per SIMD hold 256 of the 512 entries and waves of
//     another kernel fit beside it for its whole run -- the weight gradients are side-stream work that only the optimiser
//     waits for, and the HBM-bound BatchNorm tails of the main stream run beside them.  Alone the kernel
//     is 4 - 6.5 % slower than the two-workgroup form at 128->256 and 256->512 channels; it is kept for
//     what it does to the iteration.  The launch bound of 1024 threads is what gives the compiler that budget (a
//     workgroup is launched with kWgThreads = 512; see kWgLaunchBound).
//   * the workgroup hides its own staging: two LDS images (2 x 49 280 B at F = 8 / 16, 2 x 53 120 B at F = 32: more than
//     half of the CU's 160 KB, so no second workgroup of this kernel shares the CU, and room for two 17 KB workgroups of
//     the tail kernels beside it).  The next chunk is requested behind the first K-group's MFMAs, waits in registers
//     (2 + at most 4 uint4 per thread) and is stored into the other image before the last K-group; one barrier per chunk.
//   * each K slab writes its fp32 partial tile to its own workspace slot once (no atomics, no memset); a second launch
//     adds the slots in a fixed order (conv3x3_wgrad_sum_kernel) and rounds once into dW in the parameter's own layout
//     ([Cout][3][3][Cin]) and dtype.  Deterministic: the same inputs give the same bits on every call.
#include <hip/hip_bf16.h>

#include "conv3x3_image.h"
#include "seld_bf16.h"
#include "seld_common.h"

namespace seld {

namespace {

using namespace conv3x3;            // types, the staged image and the transposed reads (conv3x3_image.h)

constexpr int kWgThreads = 512;      // 8 waves: 2 (co) x 4 (ci)
constexpr int kWgTile = 64;          // output channels and input channels per workgroup
constexpr int kWgKc = 128;           // positions per staged chunk
constexpr int kWgPitch = kPitch;
constexpr int kWgSumThreads = 256;
constexpr int kWgSumRows = 8;        // slab subsets per element of the fixed-order sum

template <int F>
struct WgradGeom {
  using Img = Image<F, kWgKc>;
  static constexpr int TC = Img::TC;                         // time rows per chunk
  static constexpr int XR = Img::kRows;                      // x image rows (with halo rows and edge columns)
  static constexpr int kDyLoads = kWgKc * 8 / kWgThreads;    // 16-byte pieces per thread
  static constexpr int kXLoads = (XR * 8 + kWgThreads - 1) / kWgThreads;
  static constexpr int kRowsPerStep = 32 / F * (F + 2);       // image rows between positions p and p + 32
  static constexpr int kHighHalf = F == 32 ? 16 : 16 / F * (F + 2);      // ... between positions p and p + 16 (p < 16)
  static constexpr int kImageShorts = (kWgKc + XR) * kWgPitch;           // one chunk: dy, then the x image
  static constexpr int kLdsShorts = 2 * kImageShorts;
  // more than half of the CU's 160 KB (one workgroup of this kernel per CU), and room for two 17 KB workgroups beside it
  static_assert(kLdsShorts * 2 > 80 * 1024 && kLdsShorts * 2 <= 124 * 1024, "LDS footprint outside its bracket");
};

// The launch bound is TWICE the workgroup the kernel is launched with (launch_wgrad: kWgThreads): a bound of 16 waves is 4
// per SIMD, i.e. 512 / 4 = 128 registers per lane, which is the budget that leaves half of the register file free.
// (With a bound of kWgThreads the compiler sizes the budget by the LDS occupancy, one workgroup = 2 waves per SIMD, and
// takes up to 256; amdgpu_waves_per_eu is capped the same way.)  The budget also leans on the compiler: the piece and
// lane addresses are re-derived per chunk behind an empty asm, the K-group loop is rolled, and sched_group_barrier
// orders reads and MFMAs.  AFTER EVERY ROCm / compiler update run tests/test_conv_wgrad_occupancy_cpu.py (<= 128
// registers, no scratch, LDS bracket) and tests/test_conv_wgrad_cpu.py: they are the only guard of this.
constexpr int kWgLaunchBound = 2 * kWgThreads;
static_assert(kWgLaunchBound == 1024 && kWgLaunchBound / 64 / 4 == 4, "the register budget is 512 / (bound waves per SIMD)");

template <int F>
__global__ __launch_bounds__(kWgLaunchBound) void conv3x3_wgrad_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ dy, int T, int Cin, int Cout,
    int chunks_per_clip, int chunks, int per_slab, float* __restrict__ ws) {
  using G = WgradGeom<F>;
  __shared__ __attribute__((aligned(16))) unsigned short lds[G::kLdsShorts];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int ci0 = blockIdx.x * kWgTile, co0 = blockIdx.y * kWgTile;
  const int c_begin = blockIdx.z * per_slab;
  const int c_end = min(c_begin + per_slab, chunks);

  f32x4 acc[9][2];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int m = 0; m < 2; ++m) acc[k][m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  // The next chunk waits in registers during a chunk's MFMAs.  Loads without branches: a piece outside the map (a time
  // row outside [0, T), an edge column, the image's tail) reads the chunk's first element instead and is replaced by
  // zero when it is stored.  Addresses are a per-chunk uniform base (time row t0 of the clip, always inside) plus a
  // 32-bit lane offset that is recomputed per chunk rather than kept in registers beside the accumulators.
  uint4 rdy[G::kDyLoads], rx[G::kXLoads];
  bool in_dy[G::kDyLoads], in_x[G::kXLoads];
  auto load = [&](int c) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int b = c / chunks_per_clip, t0 = (c - b * chunks_per_clip) * G::TC;
    const long row0 = (static_cast<long>(b) * T + t0) * F;
    const unsigned short* const dy0 = dy + row0 * Cout + co0;
    const unsigned short* const x0 = x + row0 * Cin + ci0;
    const int ch8 = (tid & 7) * 8;
#pragma unroll
    for (int i = 0; i < G::kDyLoads; ++i) {
      const int pos = (tid >> 3) + i * (kWgThreads / 8);
      in_dy[i] = t0 + pos / F < T;
      rdy[i] = *reinterpret_cast<const uint4*>(dy0 + (in_dy[i] ? pos * Cout + ch8 : 0));
    }
#pragma unroll
    for (int i = 0; i < G::kXLoads; ++i) {
      const int r = (tid >> 3) + i * (kWgThreads / 8);                       // image row: (tr, f + 1)
      const int tr = r / (F + 2), f = r - tr * (F + 2) - 1, t = t0 - 1 + tr;
      in_x[i] = r < G::XR && t >= 0 && t < T && f >= 0 && f < F;
      rx[i] = *reinterpret_cast<const uint4*>(x0 + (in_x[i] ? ((tr - 1) * F + f) * Cin + ch8 : 0));
    }
  };
  auto store = [&](unsigned short* image) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    unsigned short* const ldy = image;
    unsigned short* const lx = image + kWgKc * kWgPitch;
    auto piece_or_zero = [](uint4 v, bool inside) {
      return make_uint4(inside ? v.x : 0u, inside ? v.y : 0u, inside ? v.z : 0u, inside ? v.w : 0u);
    };
#pragma unroll
    for (int i = 0; i < G::kDyLoads; ++i) {
      const int piece = tid + i * kWgThreads;
      *reinterpret_cast<uint4*>(ldy + (piece >> 3) * kWgPitch + (piece & 7) * 8) = piece_or_zero(rdy[i], in_dy[i]);
    }
#pragma unroll
    for (int i = 0; i < G::kXLoads; ++i) {
      const int piece = tid + i * kWgThreads;
      if (piece < G::XR * 8)
        *reinterpret_cast<uint4*>(lx + (piece >> 3) * kWgPitch + (piece & 7) * 8) = piece_or_zero(rx[i], in_x[i]);
    }
  };

  if (c_begin < c_end) {
    load(c_begin);
    store(lds);
  }
  for (int c = c_begin; c < c_end; ++c) {
    // chunk c's image is complete, and every wave is done reading the other image (chunk c-1)
    __syncthreads();
    // lane 4q+p of the 16-lane group g supplies row q, columns 4p..4p+3 of its 4-row block (ds_read_b64_tr_b16):
    // dy rows lpos and lpos + 16 of a K-group of 32, and the x image rows of the same positions.  lpos < 16 and F
    // divides 32, so the image row of position 32 ks + lpos (+ 16) is that of lpos plus a constant: every fragment read
    // below is one of two lane addresses (derived per chunk, not kept over the prefetch) plus a compile-time offset.
    int lt = threadIdx.x;
    asm volatile("" : "+v"(lt));
    const int g = (lt >> 4) & 3, q = (lt >> 2) & 3, p = lt & 3, wv = lt >> 6;
    const int lpos = 4 * g + q;
    const unsigned short* const image = lds + ((c - c_begin) & 1) * G::kImageShorts;
    const unsigned short* const pa = image + lpos * kWgPitch + (wv >> 2) * 32 + 4 * p;
    const unsigned short* const pb = image + (kWgKc + image_row<F>(lpos)) * kWgPitch + (wv & 3) * 16 + 4 * p;
    const bool more = c + 1 < c_end;
    unsigned short* const other = lds + ((c + 1 - c_begin) & 1) * G::kImageShorts;

    // (a rolled loop: unrolled, the compiler shares fragment halves between K-groups and taps and keeps them and the
    // next group's dy fragments live beside the accumulators and the prefetch, which then spills)
#pragma unroll 1
    for (int ks = 0; ks < kWgKc / 32; ++ks) {
      const unsigned short* const ka = pa + ks * 32 * kWgPitch;
      const unsigned short* const kb = pb + ks * G::kRowsPerStep * kWgPitch;
      bf16x8 a[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = join(tr_read(ka, m * 16), tr_read(ka, 16 * kWgPitch + m * 16));
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int row = tap_shift<F>(tap);
        const bf16x8 bfr = join(tr_read(kb, row * kWgPitch), tr_read(kb, (row + G::kHighHalf) * kWgPitch));
#pragma unroll
        for (int m = 0; m < 2; ++m)
          acc[tap][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bfr, acc[tap][m], 0, 0, 0);
      }
      // issue order: the dy fragments and two taps' x fragments, then per tap two MFMAs and the reads of a later tap
      // (all reads first would hold every tap's fragments in registers at once)
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
      // the next chunk: requested behind the first K-group's MFMAs (which start right after the barrier), in flight
      // during the next two, stored into the other image before the last, whose MFMAs cover the stores
      if (more && ks == 0) load(c + 1);
      if (more && ks == kWgKc / 32 - 2) store(other);
    }
  }

  // C/D of the 16x16 tile: column (ci) = lane & 15, rows (co) = 4 * (lane >> 4) + j
  float* const slot = ws + static_cast<long>(blockIdx.z) * Cout * 9 * Cin;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = co0 + wm * 32 + m * 16 + 4 * (lane >> 4) + j;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        slot[(static_cast<long>(co) * 9 + tap) * Cin + ci0 + wn * 16 + (lane & 15)] = acc[tap][m][j];
    }
}

// dw[i] = round(sum over s of ws[s][i]) in a fixed order: thread row r of the workgroup adds slabs r, r + 8, r + 16, ...
// of 4 consecutive elements (count % 4 == 0), then row 0 adds the 8 row sums in row order.  Eight rows in flight per
// column: the small-tile shapes have up to 256 slabs over few elements (a single thread per element there is a
// latency-bound walk: 68 us for 64->128 channels).
template <bool kBf16>
__global__ __launch_bounds__(kWgSumThreads) void conv3x3_wgrad_sum_kernel(const float* __restrict__ ws, int slabs,
                                                                           long count, void* __restrict__ dw) {
  constexpr int kCols = kWgSumThreads / kWgSumRows;
  __shared__ float4 part[kWgSumRows][kCols];
  const int col = threadIdx.x % kCols, row = threadIdx.x / kCols;
  const long i = (static_cast<long>(blockIdx.x) * kCols + col) * 4;
  float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < count)
    for (int k = row; k < slabs; k += kWgSumRows) {
      const float4 v = *reinterpret_cast<const float4*>(ws + static_cast<long>(k) * count + i);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  part[row][col] = s;
  __syncthreads();
  if (row != 0 || i >= count) return;
#pragma unroll
  for (int r = 1; r < kWgSumRows; ++r) {
    const float4 v = part[r][col];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float out[4] = {s.x, s.y, s.z, s.w};
  if (kBf16) Row<__hip_bfloat16, 4>::store(dw, i, out);
  else Row<float, 4>::store(dw, i, out);
}

struct WgradPlan {
  int chunks_per_clip = 0, chunks = 0, per_slab = 0, slabs = 0;
};

int time_rows_per_chunk(int64_t F) { return static_cast<int>(kWgKc / F); }

bool wgrad_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return (F == 8 || F == 16 || F == 32) && Cin > 0 && Cout > 0 && Cin % kWgTile == 0 &&
         Cout % kWgTile == 0;
}

// K slabs: enough workgroups for one per CU, each slab at least one chunk
WgradPlan wgrad_plan(int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout, int num_cus) {
  WgradPlan pl;
  const int tc = time_rows_per_chunk(F);
  pl.chunks_per_clip = static_cast<int>((T + tc - 1) / tc);
  pl.chunks = static_cast<int>(B) * pl.chunks_per_clip;
  const long tiles = (Cin / kWgTile) * (Cout / kWgTile);
  const long want = ((num_cus > 0 ? num_cus : 256) + tiles - 1) / tiles;
  const long slabs = want < 1 ? 1 : (want > pl.chunks ? pl.chunks : want);
  pl.per_slab = static_cast<int>((pl.chunks + slabs - 1) / slabs);
  pl.slabs = (pl.chunks + pl.per_slab - 1) / pl.per_slab;
  return pl;
}

template <int F>
void launch_wgrad(const unsigned short* x, const unsigned short* dy, int T, int Cin, int Cout, const WgradPlan& pl,
                  float* ws, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(Cin / kWgTile), static_cast<unsigned>(Cout / kWgTile),
                  static_cast<unsigned>(pl.slabs));
  hipLaunchKernelGGL(conv3x3_wgrad_kernel<F>, grid, dim3(kWgThreads), 0, stream, x, dy, T, Cin, Cout,
                     pl.chunks_per_clip, pl.chunks, pl.per_slab, ws);
}

}  // namespace

}  // namespace seld

extern "C" {

int seld_conv3x3_wgrad_supported(int64_t F, int64_t Cin, int64_t Cout) {
  return seld::wgrad_supported(F, Cin, Cout) ? 1 : 0;
}

int64_t seld_conv3x3_wgrad_workspace_floats(int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st || B <= 0 || T <= 0 || !wgrad_supported(F, Cin, Cout)) return 0;
  return static_cast<int64_t>(wgrad_plan(B, T, F, Cin, Cout, st->num_cus).slabs) * Cout * 9 * Cin;
}

int seld_conv3x3_wgrad(const void* x, const void* dy, int64_t B, int64_t T, int64_t F, int64_t Cin, int64_t Cout,
                       void* dw, int dw_is_bf16, float* workspace, void* stream_) {
  using namespace seld;
  const DeviceState* st = current_state();
  if (!st) return kErrNotInitialised;
  if (!x || !dy || !dw || !workspace || B <= 0 || T <= 0)
    return fail(kErrInvalidArgument, "seld_conv3x3_wgrad: bad argument");
  if (!wgrad_supported(F, Cin, Cout))
    return fail(kErrUnsupported, "seld_conv3x3_wgrad: F in {8, 16, 32} and channel counts % 64 == 0 required");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dw) |
        reinterpret_cast<uintptr_t>(workspace)) & 15) != 0)
    return fail(kErrInvalidArgument, "seld_conv3x3_wgrad: 16-byte aligned tensors required");
  const WgradPlan pl = wgrad_plan(B, T, F, Cin, Cout, st->num_cus);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const unsigned short* xs = static_cast<const unsigned short*>(x);
  const unsigned short* ds = static_cast<const unsigned short*>(dy);
  const int t = static_cast<int>(T), ci = static_cast<int>(Cin), co = static_cast<int>(Cout);
  switch (F) {
    case 8: launch_wgrad<8>(xs, ds, t, ci, co, pl, workspace, stream); break;
    case 16: launch_wgrad<16>(xs, ds, t, ci, co, pl, workspace, stream); break;
    default: launch_wgrad<32>(xs, ds, t, ci, co, pl, workspace, stream); break;
  }
  SELD_HIP_TRY(hipGetLastError());
  const long count = static_cast<long>(Cout) * 9 * Cin;
  const long cols = kWgSumThreads / kWgSumRows;
  const dim3 grid(static_cast<unsigned>((count / 4 + cols - 1) / cols));
  if (dw_is_bf16)
    hipLaunchKernelGGL(conv3x3_wgrad_sum_kernel<true>, grid, dim3(kWgSumThreads), 0, stream, workspace, pl.slabs,
                       count, dw);
  else
    hipLaunchKernelGGL(conv3x3_wgrad_sum_kernel<false>, grid, dim3(kWgSumThreads), 0, stream, workspace, pl.slabs,
                       count, dw);
  SELD_HIP_TRY(hipGetLastError());
  return kOk;
}

}  // extern "C"
